"""The summation orders and the tie rule of csrc/wave_ops.h pinned to their kernels on the MI355X: every entry
below takes caller-supplied buffers and stores a result in which the sum's own precision is still visible, and that result is
compared BIT FOR BIT with the numpy emulation of the documented order (tests/wave_order.py).

    tts_sumsq              256-entry LDS tree              the caller's partials, and the norm
    tts_stoi_reduce        butterfly + left fold, fp64     totals (one-barrier form: wave_sum and fold_left on the kernel's own red)
    tts_stoi_frame_energy  butterfly of one wavefront      energy
    tts_activity_level     in-order walk, fp64             sums[2u]
    tts_prosody_control    butterfly + left fold, fp32     every row of pitch and energy, through the mean
    tts_prominence_units   butterfly of one wavefront      rows[:, 2]; the tie rule of wave_arg_max / wave_arg_min in columns 1 and 7
    tts_pitch_path         wave_arg_max<16>                the back-pointer bytes in the caller's scratch

The inputs come from tests/wave_order_cases.py, whose builders assert on the host, before the GPU is touched, that each case tells
its order from the other two (tests/test_wave_order_cpu.py runs the same builders without a GPU).  Everything a kernel must not read
is NaN or junk.  A change of order in a kernel must change the emulation here with it."""
import functools

import numpy as np
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import capi
from tests import wave_order as wo
from tests import wave_order_cases as wc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def same_bits(got, want):
    return np.array_equal(wo.bits(np.asarray(got)), wo.bits(np.asarray(want)))


# ---- tts_sumsq ---------------------------------------------------------------------------------------------------------------------
def run_sumsq(x, lead=0):
    """x at offset ``lead`` of a buffer that is NaN around it -> (partials float64 [256], norm float32)."""
    buf = np.full(lead + len(x) + 3, np.nan, dtype=F32)
    buf[lead: lead + len(x)] = x
    xd = dv(buf)
    partials = torch.full((capi.SUMSQ_PARTIALS,), float("nan"), dtype=torch.float64, device=DEV)
    norm = torch.full((1,), float("nan"), dtype=torch.float32, device=DEV)
    capi.check(capi.lib().tts_sumsq(xd[lead:].data_ptr(), len(x), partials.data_ptr(), norm.data_ptr(), stream()), "tts_sumsq")
    torch.cuda.synchronize()
    return partials.cpu().numpy(), norm.cpu().numpy()[0]


@pytest.mark.parametrize("n", wc.SUMSQ_N)
def test_sumsq_adds_in_the_tree_order(n):
    """Workgroup b owns x[b chunk : (b + 1) chunk], chunk = ceil(n / 256); thread t adds the fp64 squares (exact, so a fused
    multiply-add changes nothing) of its elements t, t + 256, ... in turn; then the 256-entry tree.  All 256 partials are pinned,
    and the norm is float32(sqrt(tree(partials))): fp64 sqrt and the cast are both correctly rounded on the MI355X as in numpy, so
    it is pinned bit for bit as well."""
    x, partials, norm = wc.sumsq_case(n)
    assert capi.SUMSQ_PARTIALS == wc.PARTIALS
    got_partials, got_norm = run_sumsq(x)
    differ = np.flatnonzero(wo.bits(got_partials) != wo.bits(partials))
    ulps = abs(int(wo.bits(got_norm)[0]) - int(wo.bits(norm)[0]))
    print(f"n {n}: {len(differ)} of 256 partials differ; norm {got_norm!r} against {norm!r}: {ulps} ulp")
    assert len(differ) == 0, (differ[:8], got_partials[differ[:8]], partials[differ[:8]])
    assert ulps == 0


# ---- tts_stoi_reduce ---------------------------------------------------------------------------------------------------------------
def run_stoi(cases, frames=()):
    """One launch over the pairs of ``cases`` (segment values [S, 2], M = S + 29 frames) and then pairs of ``frames`` frames without
    values -> totals float64 [pairs, 2].  What lies past a pair's segments is NaN."""
    M = [len(c) + wc.STOI_SEG - 1 for c in cases] + list(frames)
    max_frames = max(max(M), 1)
    max_segments = max(1, max_frames - (wc.STOI_SEG - 1))
    seg = np.full((len(M), max_segments, 2), np.nan, dtype=F64)
    for k, c in enumerate(cases):
        seg[k, : len(c)] = c
    sd, cd = dv(seg), dv(np.asarray(M, dtype=np.int32))
    totals = torch.full((len(M), 2), 5.0, dtype=torch.float64, device=DEV)
    capi.check(capi.lib().tts_stoi_reduce(sd.data_ptr(), cd.data_ptr(), len(M), max_frames, totals.data_ptr(), stream()), "tts_stoi_reduce")
    torch.cuda.synchronize()
    return totals.cpu().numpy()


@functools.lru_cache(maxsize=None)
def stoi_batch():
    return run_stoi([wc.stoi_case(S)[0] for S in wc.STOI_SEGMENTS], frames=(29, 0, 1))


def test_stoi_reduce_adds_in_the_butterfly_order():
    """Per pair and column: thread t of 256 adds segments t, t + 256, ... in turn, wave_sum, the four wavefronts left to right
    (include/toucan_intelligibility.h), divided by S = M - 29.  A pair of fewer than 30 frames still gives NaN."""
    want = np.stack([wc.stoi_case(S)[1] for S in wc.STOI_SEGMENTS])
    got = stoi_batch()
    assert same_bits(got[: len(want)], want), (got, want)
    assert np.isnan(got[len(want):]).all()


# ---- tts_stoi_frame_energy ---------------------------------------------------------------------------------------------------------
def run_stoi_energy(waves, lead=3):
    """One launch over pairs whose recording is one of ``waves`` (NaN in front of each and behind the last; the generated side is
    not read) -> energy float64 [pairs, max_frames], NaN where the kernel wrote nothing."""
    parts, pairs, at = [], [], 0
    for x in waves:
        parts += [np.full(lead, np.nan, dtype=F32), x]
        pairs.append((at + lead, at + lead, len(x)))
        at += lead + len(x)
    buf = np.concatenate(parts + [np.full(lead, np.nan, dtype=F32)])
    pairs = np.asarray(pairs, dtype=np.int64)
    max_frames = max((len(x) - wc.STOI_N) // wc.STOI_HOP + 1 for x in waves) + 1
    xd, pd, wd = dv(buf), dv(pairs), dv(wc.stoi_window())
    energy = torch.full((len(waves), max_frames), float("nan"), dtype=torch.float64, device=DEV)
    capi.check(capi.lib().tts_stoi_frame_energy(xd.data_ptr(), len(buf), pd.data_ptr(), pairs.ctypes.data, len(waves), wd.data_ptr(), max_frames,
                                                energy.data_ptr(), stream()), "tts_stoi_frame_energy")
    torch.cuda.synchronize()
    return energy.cpu().numpy()


@functools.lru_cache(maxsize=None)
def stoi_energy_batch():
    return run_stoi_energy([wc.stoi_energy_case(F)[0] for F in wc.STOI_ENERGY_FRAMES])


def test_stoi_frame_energy_adds_in_the_wavefront_order():
    """energy[p][f]: the fp32 products w x (one rounding), their squares (exact) and the sum in fp64; lane l adds samples l, l + 64,
    l + 128, l + 192 of the frame in turn, then wave_sum (include/toucan_intelligibility.h).  Pairs of five frames (one more than
    a workgroup takes) and of two; the slots past a pair's frames are not written."""
    got = stoi_energy_batch()
    for k, F in enumerate(wc.STOI_ENERGY_FRAMES):
        want = wc.stoi_energy_case(F)[1]
        assert same_bits(got[k, :F], want), (F, got[k, :F], want)
        assert np.isnan(got[k, F:]).all()


# ---- tts_activity_level ------------------------------------------------------------------------------------------------------------
ACTIVITY_S = 800  # samples of a slot at 8 kHz, the smallest rate


def run_activity(cases, max_segments):
    """One launch over utterances whose slots hold the sq values of ``cases`` (the last slot of every other utterance partial), pos
    all -1, a peak per slot; the slots past an utterance's own are NaN (sq) and huge (peak) -> (sums [B, 2], counts, stats, peaks)."""
    B, S = len(cases), ACTIVITY_S
    spans, at = [], 7
    for u, c in enumerate(cases):
        count = len(c) * S - (37 if u % 2 else 0)
        spans.append((at, count))
        at += count + 11
    sq = np.full((B, max_segments), np.nan, dtype=F64)
    peak = np.full((B, max_segments), 1e30, dtype=F32)
    rng = np.random.default_rng(B)
    for u, c in enumerate(cases):
        assert len(c) <= max_segments
        sq[u, : len(c)] = c
        peak[u, : len(c)] = rng.random(len(c)).astype(F32)
    pos = np.full((B, max_segments, 32), -1, dtype=np.int32)
    sqd, pkd, posd, spd = dv(sq), dv(peak), dv(pos), dv(np.asarray(spans, dtype=np.int64))
    counts = torch.full((B, capi.ACTIVITY_COUNTS), -5, dtype=torch.int64, device=DEV)
    sums = torch.full((B, 2), float("nan"), dtype=torch.float64, device=DEV)
    stats = torch.full((B, capi.ACTIVITY_N_COLUMNS), float("nan"), dtype=torch.float64, device=DEV)
    capi.check(capi.lib().tts_activity_level(sqd.data_ptr(), pkd.data_ptr(), posd.data_ptr(), at, spd.data_ptr(), B, S, max_segments, float("nan"), 0.0,
                                             counts.data_ptr(), sums.data_ptr(), stats.data_ptr(), stream()), "tts_activity_level")
    torch.cuda.synchronize()
    peaks = np.array([peak[u, : len(c)].max() for u, c in enumerate(cases)], dtype=F64)
    return sums.cpu().numpy(), counts.cpu().numpy(), stats.cpu().numpy(), peaks


@functools.lru_cache(maxsize=None)
def activity_batch():
    return run_activity([wc.activity_case(k)[0] for k in wc.ACTIVITY_SLOTS], max(wc.ACTIVITY_SLOTS) + 2)


def test_activity_level_adds_in_slot_order():
    """sums[2u] is the plain sequential sum of the utterance's sq slots (wave_each_in_order: 64 slots loaded by the lanes, added in
    index order).  The utterances differ in length and NaN lies behind each one's slots, so a walk that ran on shows.  With no
    sample at any threshold there is no level: the counts are 0, the levels -inf, the gain 1; the peak is the largest of the slots."""
    want = np.array([wc.activity_case(k)[1] for k in wc.ACTIVITY_SLOTS])
    sums, counts, stats, peaks = activity_batch()
    assert same_bits(sums[:, 0], want), (sums[:, 0], want)
    assert np.array_equal(sums[:, 1], peaks)
    assert not counts[:, :15].any() and np.isneginf(stats[:, [0, 1, 3, 7]]).all() and (stats[:, 6] == 1.0).all()


# ---- tts_prosody_control -----------------------------------------------------------------------------------------------------------
def run_prosody(cases, gap=3):
    """One launch of the scalar entry (duration 1, pitch 2, energy 2, pause 1) over utterances whose rows hold ``cases`` (float32
    [n, 2]: pitch, energy), ``gap`` rows of NaN in front of each and behind the last.  Every other zero of a case is made by the
    kernel's own override (voiced / phoneme flag 0 over a NaN) instead of being given -> (rows after the call per case, ok)."""
    total = gap + sum(len(c) + gap for c in cases)
    text = np.full((total, 64), np.nan, dtype=F32)
    pe = np.full((total, 2), np.nan, dtype=F32)
    dur = np.arange(total, dtype=np.int32) % 9
    sb, se, at = [], [], gap
    for c in cases:
        n = len(c)
        sb.append(at), se.append(at + n)
        t = text[at: at + n]
        t[:] = 0.0
        t[:, [15, 61]] = 1.0
        pe[at: at + n] = c
        for col, flag in ((0, 61), (1, 15)):
            zeros = np.flatnonzero(c[:, col] == 0)[::2]
            t[zeros, flag] = 0.0
            pe[at + zeros, col] = np.nan
        at += n + gap
    before = pe.copy()
    td, pd, ed, dd = dv(text), dv(pe[:, 0]), dv(pe[:, 1]), dv(dur)
    sbd, sed = dv(np.asarray(sb, dtype=np.int32)), dv(np.asarray(se, dtype=np.int32))
    capi.check(capi.lib().tts_prosody_control(td.data_ptr(), 64, pd.data_ptr(), ed.data_ptr(), dd.data_ptr(), sbd.data_ptr(), sed.data_ptr(), len(cases),
                                              1.0, wc.PROSODY_SCALE, wc.PROSODY_SCALE, 1.0, stream()), "tts_prosody_control")
    torch.cuda.synchronize()
    after = np.stack([pd.cpu().numpy(), ed.cpu().numpy()], axis=1)
    inside = np.zeros(total, dtype=bool)
    for b, e in zip(sb, se):
        inside[b:e] = True
    ok = same_bits(after[~inside], before[~inside]) and np.array_equal(dd.cpu().numpy(), dur)  # the gaps and the durations are as they were
    return [after[b:e].copy() for b, e in zip(sb, se)], ok


@functools.lru_cache(maxsize=None)
def prosody_batch():
    return run_prosody([wc.prosody_case(r)[0] for r in wc.PROSODY_ROWS])


def test_prosody_control_model_is_exact_where_the_order_cannot_matter():
    """Seven non-zero powers of two among 300 rows: their fp32 sum is exact in any order, so this compares the float32 numpy model of
    the arithmetic around the sum (count, division, shift, doubling, shift back, clamp) with the kernel and nothing else.  A
    mismatch in the next test is then the order's."""
    v, want = wc.prosody_exact_case()
    got, ok = run_prosody([v], gap=2)
    assert ok and same_bits(got[0], want), (got[0][:8], want[:8])


def test_prosody_control_adds_in_the_butterfly_order():
    """The mean of the non-zero rows is block_sum of the strided-256 fp32 sums over the fp32 count.  With a scale of exactly 2 and
    no curves every stored row is ((v - avg) * 2) + avg clamped at 0, fused or not, and shows the bits of avg; the cases' stored
    rows differ between the orders in both columns (asserted by the builder)."""
    got, ok = prosody_batch()
    assert ok
    for r, g in zip(wc.PROSODY_ROWS, got):
        want = wc.prosody_case(r)[1]
        assert same_bits(g, want), (r, np.flatnonzero((wo.bits(g) != wo.bits(want)).any(axis=1))[:8])


# ---- tts_prominence_units ------------------------------------------------------------------------------------------------------------
BAND = 2  # j_lo == j_hi: the composite is w[0][BAND] alone


def run_units(utterances, lead=2):
    """utterances: [(w0 float64 [T], [(b, e) ...])] -> rows float64 [units, 8] per utterance.  Weights (1, 0, 0) and one scale: the
    composite is (1 * (0 + w0) + 0 * junk) + 0 * junk = w0 exactly.  The other two channels hold finite junk at that scale (0 * NaN
    would be NaN); every other scale and every frame outside the utterances is NaN."""
    total = lead + sum(len(w0) + lead for w0, _ in utterances)
    w = np.full((capi.PROMINENCE_CHANNELS, capi.PROMINENCE_SCALES, total), np.nan, dtype=F64)
    utts, units, at = [], [], lead
    for w0, un in utterances:
        T = len(w0)
        w[0, BAND, at: at + T] = w0
        w[1, BAND, at: at + T], w[2, BAND, at: at + T] = 7.0, -3.0
        utts.append((at, T, 0, 0, len(units), len(un)))
        units += list(un)
        at += T + lead
    utts, units = np.asarray(utts, dtype=np.int64), np.asarray(units, dtype=np.int32).reshape(-1, 2)
    wd, ud, nd = dv(w), dv(utts), dv(units)
    rows = torch.full((len(units), capi.PROMINENCE_N_COLUMNS), 99.0, dtype=torch.float64, device=DEV)
    capi.check(capi.lib().tts_prominence_units(wd.data_ptr(), total, ud.data_ptr(), utts.ctypes.data, len(utts), nd.data_ptr(), units.ctypes.data, len(units),
                                               1.0, 0.0, 0.0, BAND, BAND, rows.data_ptr(), None, stream()), "tts_prominence_units")
    torch.cuda.synchronize()
    rows = rows.cpu().numpy()
    return [rows[u[4]: u[4] + u[5]].copy() for u in utts]


def unit_utterances():
    """Two utterances of different lengths: units of 1, 63, 200, 64 and 65 frames (more units than the workgroup has wavefronts)
    with NaN frames between them, and units of 130 and 3 frames."""
    def lay(values, first):
        parts, units, at = [np.full(first, np.nan)], [], first
        for v in values:
            units.append((at, at + len(v)))
            parts += [v, np.full(2, np.nan)]
            at += len(v) + 2
        return np.concatenate(parts), units

    rng = np.random.default_rng(24)
    a = [wc.unit_case(f)[0] for f in (1, 63, 200, 64, 65)]
    b = [wo.wide_values(rng, (130,), F64), wo.wide_values(rng, (3,), F64)]
    return [lay(a, 3), lay(b, 0)], [a, b]


@functools.lru_cache(maxsize=None)
def units_batch():
    return run_units(unit_utterances()[0])


def test_prominence_units_add_in_the_wavefront_order():
    """rows[:, 2]: lane l adds the composite of frames b + l, b + l + 64, ... in turn, wave_sum (the butterfly alone: one wavefront
    per unit), divided by e - b.  Columns 0, 1, 3: the maximum, its frame, its pitch part; 4, 5: the zero-weight parts."""
    utterances, values = unit_utterances()
    got = units_batch()
    for (w0, units), vals, rows in zip(utterances, values, got):
        for (b, e), v, row in zip(units, vals, rows):
            mean = wo.butterfly_order_sum(v, F64, threads=64) / F64(len(v))
            assert same_bits(row[2], mean), (len(v), row[2], mean)
            assert row[0] == v.max() == row[3] and row[1] == b + int(np.argmax(v)) and row[4] == 0.0 and row[5] == 0.0
    for f, row in zip((1, 63, 200, 64, 65), got[0]):
        assert same_bits(row[2], wc.unit_case(f)[1])  # the value the builder told apart from the sequential sum


def test_prominence_units_keep_the_first_of_equal_values():
    """The tie rule of wave_arg_max and wave_arg_min (better, or equal and the smaller index) with planted plateaus: equal maxima at
    frames b + 63 and b + 64 (the lower index sits in the higher lane), at b + 5 and b + 64 + 5 (one lane, two strides), and an
    all-equal unit: column 1 is the first frame.  The same three for the valley between two peaks, whose scan starts at the first
    peak: column 7 is the first minimum."""
    utterances, want = [], []
    for name, v, first in wc.plateau_cases(True):
        w0 = np.full(170, np.nan)
        w0[7: 7 + len(v)] = v
        utterances.append((w0, [(7, 7 + len(v))]))
        want.append((name, 1, wo.arg_best(v, 64, True, first=7)))
        assert want[-1][2] == (v[first], 7 + first)
    for name, v, first in wc.plateau_cases(False):
        v = v.copy()
        if name != "all equal":
            v[0], v[-1] = 9.0, 9.5  # the two peaks; between them the plateau is the minimum
        w0 = np.full(160, np.nan)
        w0[4: 4 + len(v)] = v
        frm, to = 4, 4 + len(v) - (1 if name != "all equal" else 4)  # all equal: the second peak is its unit's first frame
        utterances.append((w0, [(4, 8), (4 + len(v) - 4, 4 + len(v))]))
        want.append((name, 7, wo.arg_best(w0[frm: to + 1], 64, False, first=frm)))
        assert want[-1][2] == (v[first], 4 + first) and first == int(np.argmin(w0[frm: to + 1]))
    got = run_units(utterances)
    for (name, col, (value, frame)), rows, (w0, units) in zip(want, got, utterances):
        if col == 1:
            assert (rows[0][0], rows[0][1]) == (value, frame), (name, rows[0])
        else:
            assert (rows[0][1], rows[1][1]) == (units[0][0], units[1][0] if name == "all equal" else units[1][1] - 1), (name, rows)
            assert (rows[0][6], rows[0][7]) == (-value, frame), (name, rows[0])
            assert np.isnan(rows[1][6]) and rows[1][7] == -1.0  # no peak to the right of the last unit


# ---- tts_pitch_path --------------------------------------------------------------------------------------------------------------------
def run_path(cases):
    """One launch over utterances of voiceless candidates (frequency 0) with the given strengths, all back-pointers in the caller's
    scratch (lds_frames = 0, every offset >= 0).  The candidates past a frame's n_cand are NaN; a NaN row lies between the utterances
    and 16 bytes of junk between their scratch areas -> (scratch rows uint8 [T, 16] per case, f0 per case, junk untouched)."""
    rows = sum(len(s) + 1 for _, s, _, _ in cases)
    freq = np.full((rows, wc.CANDIDATES), np.nan, dtype=F32)
    strength = np.full((rows, wc.CANDIDATES), np.nan, dtype=F32)
    n_cand = np.zeros(rows, dtype=np.int32)
    fb, nf, off, at, sat = [], [], [], 0, wc.PATH_ROW
    for _, s, nc, _ in cases:
        T = len(s)
        for t in range(T):
            freq[at + t, : nc[t]] = 0.0
            strength[at + t, : nc[t]] = s[t, : nc[t]]
        n_cand[at: at + T] = nc
        fb.append(at), nf.append(T), off.append(sat)
        at += T + 1
        sat += (T + 1) * wc.PATH_ROW
    scratch = torch.full((sat,), wc.UNWRITTEN, dtype=torch.uint8, device=DEV)
    f0 = torch.full((rows,), 7.0, dtype=torch.float32, device=DEV)
    fd, sd, ncd = dv(freq), dv(strength), dv(n_cand)
    fbd, nfd, offd = dv(np.asarray(fb, dtype=np.int32)), dv(np.asarray(nf, dtype=np.int32)), dv(np.asarray(off, dtype=np.int64))
    capi.check(capi.lib().tts_pitch_path(fd.data_ptr(), sd.data_ptr(), ncd.data_ptr(), fbd.data_ptr(), nfd.data_ptr(), offd.data_ptr(), scratch.data_ptr(),
                                         len(cases), 0, f0.data_ptr(), stream()), "tts_pitch_path")
    torch.cuda.synchronize()
    sc, f0 = scratch.cpu().numpy(), f0.cpu().numpy()
    used = np.zeros(sat, dtype=bool)
    for o, T in zip(off, nf):
        used[o: o + T * wc.PATH_ROW] = True
    inside = np.zeros(rows, dtype=bool)
    for b, T in zip(fb, nf):
        inside[b: b + T] = True
    clean = bool((sc[~used] == wc.UNWRITTEN).all() and (f0[~inside] == 7.0).all())
    return [sc[o: o + T * wc.PATH_ROW].reshape(T, wc.PATH_ROW).copy() for o, T in zip(off, nf)], [f0[b: b + T].copy() for b, T in zip(fb, nf)], clean


def test_pitch_path_keeps_the_first_of_equal_predecessors():
    """The scratch contract (csrc/pitch.hip, include/toucan_pitch.h): one byte per candidate, 16 per frame, byte 15 the chosen
    candidate.  Voiceless candidates of equal strength make every transition cost 0 and every predecessor tie: byte c of every
    frame's row is 0; with candidate 0 strictly worse and 3 and 9 tied it is 3; with 8 and 9 tied (the two halves of the 16 lanes
    meet at the first butterfly step) it is 8; also with fewer candidates than 15 in some frames.  The last frame's candidates tie
    as well and the serial pick keeps the first, so byte 15 of every row is the same byte.  All of f0 is 0 (voiceless)."""
    cases = wc.path_cases()
    rows, f0, clean = run_path(cases)
    assert clean
    for (name, s, nc, byte), got, f in zip(cases, rows, f0):
        want = wc.path_bytes(s, nc)
        assert np.array_equal(got[1:, : wc.CANDIDATES], want[1:, : wc.CANDIDATES]) and (got[1:, : wc.CANDIDATES] == byte).all(), (name, got)
        assert np.array_equal(got[:, 15], want[:, 15]) and (got[:, 15] == byte).all(), (name, got[:, 15])
        assert not f.any(), name


# ---- alone == in a batch -----------------------------------------------------------------------------------------------------------
def test_every_entry_alone_equals_the_ragged_batch():
    """At the raw entries what the feature tests promise: each case of the tests above alone, in buffers of its own size, gives the
    bits it gave inside the ragged batch (tts_sumsq has no batch: the same values at another offset of a larger buffer)."""
    x = wc.sumsq_case(65537)[0]
    (p0, n0), (p5, n5) = run_sumsq(x), run_sumsq(x, lead=5)
    assert same_bits(p5, p0) and same_bits(n5, n0)
    for k, S in enumerate(wc.STOI_SEGMENTS):
        assert same_bits(run_stoi([wc.stoi_case(S)[0]])[0], stoi_batch()[k]), S
    for k, F in enumerate(wc.STOI_ENERGY_FRAMES):
        assert same_bits(run_stoi_energy([wc.stoi_energy_case(F)[0]], lead=0)[0, :F], stoi_energy_batch()[k, :F]), F
    for k, slots in enumerate(wc.ACTIVITY_SLOTS):
        alone = run_activity([wc.activity_case(slots)[0]], slots)
        assert same_bits(alone[0][0, 0], activity_batch()[0][k, 0]), slots
    for k, r in enumerate(wc.PROSODY_ROWS):
        got, ok = run_prosody([wc.prosody_case(r)[0]], gap=0)
        assert ok and same_bits(got[0], prosody_batch()[0][k]), r
    for (w0, units), rows in zip(unit_utterances()[0], units_batch()):
        for (b, e), row in zip(units, rows):
            alone = run_units([(w0[b:e].copy(), [(0, e - b)])], lead=0)[0][0]
            assert same_bits(alone[[0, 2, 3]], row[[0, 2, 3]]) and alone[1] == row[1] - b, (b, e)
    cases = wc.path_cases()
    batch = run_path(cases)[0]
    for c, rows in zip(cases, batch):
        alone = run_path([c])[0][0]
        assert np.array_equal(alone[1:], rows[1:]) and np.array_equal(alone[:, 15], rows[:, 15]), c[0]
