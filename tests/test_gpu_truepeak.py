"""The delivery meter (csrc/truepeak.hip) on the MI355X: the true peak bit for bit against the materialised resampling and within
the derived bound of the float64 restatement (tests/truepeak_ref.py), a ragged batch - with gaps between the spans that hold
full-scale junk - against its utterances alone bit for bit, the loudness range's counts and order statistics exactly, the gain under
a true-peak ceiling, the limiter against its restatement, and the interface's ``true_peak_ceiling`` / ``limiter`` keywords.

The figures measured on the MI355X are recorded in DESIGN.md section 20."""
import functools
import math

import numpy as np
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import capi, interface, loudness, resample, truepeak
from tests import loudness_ref as lr
from tests import truepeak_ref as tr

pytestmark = pytest.mark.gpu
DEV = "cuda"
CEILING = -1.0
C = 10.0 ** (CEILING / 20.0)
COL = {name: i for i, name in enumerate(truepeak.RANGE_COLUMNS)}
LCOL = {name: i for i, name in enumerate(loudness.LOUDNESS_COLUMNS)}
MCOL = {name: i for i, name in enumerate(truepeak.LIMITER_COLUMNS)}
JUNK = 0.97  # what lies between the spans of a packed wave: a halo read across an utterance's edge picks it up


@functools.lru_cache(maxsize=None)
def meter():
    return truepeak.DeliveryMeter(DEV)


@functools.lru_cache(maxsize=None)
def resampler():
    return resample.Resampler(DEV)


def tile():
    return int(capi.lib().tts_truepeak_tile_samples())


def pack(waves, gap=0):
    """The waves one after the other with ``gap`` samples of junk in front of each and behind the last -> (packed on the device, spans)."""
    parts, spans, at = [], [], 0
    for i, x in enumerate(waves):
        parts.append(np.full(gap, JUNK if i % 2 else -JUNK, dtype=np.float32))
        at += gap
        spans.append((at, len(x)))
        parts.append(np.asarray(x, dtype=np.float32))
        at += len(x)
    parts.append(np.full(gap, JUNK, dtype=np.float32))
    return torch.from_numpy(np.concatenate(parts)).to(DEV), spans


def measure(waves, sr, gap=0):
    """-> float64 [B, 12] rows (RANGE_COLUMNS) of ONE ragged launch."""
    packed, spans = pack(waves, gap)
    m = meter()
    got = m.measure(packed, spans, sr)
    assert got.shape == (len(waves), 8) and got.dtype == torch.float64 and got.is_cuda
    return m.last_range.cpu().numpy().copy()


def materialised(x, sr):
    """max |.| of the utterance resampled to F sr by the resampler's kernel: the same chains, written to memory."""
    if len(x) == 0:
        return 0.0
    F = tr.factor(sr)
    y, spans = resampler().resample(torch.from_numpy(np.array(x, dtype=np.float32)).to(DEV), [(0, len(x))], sr, F * sr)
    assert spans == [(0, F * len(x))]
    return float(y.abs().max().cpu())


@functools.lru_cache(maxsize=None)
def peak_batch(sr, reverse=False, gap=0):
    cases = tr.peak_cases(tile(), sr)
    order = list(reversed(range(len(cases)))) if reverse else list(range(len(cases)))
    got = measure([cases[i]["x"] for i in order], sr, gap)
    return [got[order.index(i)] for i in range(len(cases))]


def test_the_tile_and_the_lengths_aim_at_its_edges():
    T = tile()
    assert T == 1024 and meter().tile_samples == T
    names = {c["name"]: c["n"] for c in tr.peak_cases(T)}
    assert [names[f"noise_{k}"] for k in ("T-1", "T", "T+1", "2T+1")] == [T - 1, T, T + 1, 2 * T + 1]
    assert [names[f"noise_{n}"] for n in (0, 1, 6, 7, 8, 14, 15, 16)] == [0, 1, 6, 7, 8, 14, 15, 16]
    gap = next(c for c in tr.peak_cases(T) if c["name"] == "peak_in_the_gap_at_a_tile_edge")
    o = np.abs(tr.oversample(gap["x"], 4))
    assert 4 * (T - 1) < int(o.argmax()) < 4 * T  # between the last sample of the first tile and the first of the second


@pytest.mark.parametrize("sr", (8000, 24000))
def test_true_peak_against_the_materialised_path_and_the_restatement(sr):
    """Bit-equal to max |.| of Resampler.resample(x, fs, 4 fs) per utterance - both run the same chain on the GPU - and within
    gamma_15 A max |x| of the float64 sum; the sample peak exact; dBTP = 20 log10."""
    worst = 0.0
    for c, row in zip(tr.peak_cases(tile(), sr), peak_batch(sr)):
        got = float(row[COL["true_peak"]])
        assert got == float(np.float32(got)) and got == materialised(c["x"], sr), (c["name"], got)
        assert abs(got - c["true_peak"]) <= c["bound"], (c["name"], got, c["true_peak"], c["bound"])
        worst = max(worst, abs(got - c["true_peak"]) / c["bound"] if c["bound"] else 0.0)
        assert row[COL["sample_peak"]] == c["sample_peak"], c["name"]
        assert row[COL["true_peak_dbtp"]] == (-math.inf if got == 0 else row[COL["true_peak_dbtp"]])
        if got:
            assert abs(row[COL["true_peak_dbtp"]] - 20.0 * math.log10(got)) < 1e-12
        if c["n"] == 0:
            assert got == 0.0 and row[COL["sample_peak"]] == 0.0
    by = {c["name"]: r for c, r in zip(tr.peak_cases(tile(), sr), peak_batch(sr))}
    assert by["sine_fs4_45"][COL["true_peak_dbtp"]] - tr.db(by["sine_fs4_45"][COL["sample_peak"]]) >= 2.9
    assert by["peak_in_the_gap_at_a_tile_edge"][COL["true_peak"]] > 1.2 * by["peak_in_the_gap_at_a_tile_edge"][COL["sample_peak"]]
    print(f"{sr} Hz: worst |true peak - float64| / bound {worst:.3e}")


@pytest.mark.parametrize("sr", (96000, 192000))
def test_true_peak_at_the_rates_with_other_factors(sr):
    """F = 2 at 96 kHz and F = 1 at 192 kHz (the reading is then the sample peak): the same checks on a few of the cases."""
    cases = [c for c in tr.peak_cases(tile()) if c["name"] in ("noise_T+1", "click", "noise_7", "peak_in_the_gap_at_a_tile_edge", "noise_0")]
    rows = measure([c["x"] for c in cases], sr, gap=9)
    for c, row in zip(cases, rows):
        got = float(row[COL["true_peak"]])
        assert got == materialised(c["x"], sr) and abs(got - tr.true_peak(c["x"], sr)) <= tr.bound(c["x"], sr), (c["name"], got)
        assert row[COL["sample_peak"]] == c["sample_peak"] and (sr != 192000 or got == c["sample_peak"])
        assert np.array_equal(row, measure([c["x"]], sr)[0], equal_nan=True), c["name"]


@pytest.mark.parametrize("sr", (8000, 24000))
def test_ragged_batch_equals_each_utterance_alone(sr):
    """Bit for bit in every column: packed tight, reversed, and with 37 samples of full-scale junk between the spans."""
    variants = (peak_batch(sr), peak_batch(sr, True), peak_batch(sr, False, 37), peak_batch(sr, True, 5))
    for i, c in enumerate(tr.peak_cases(tile(), sr)):
        alone = measure([c["x"]], sr)[0]
        for v in variants:
            assert np.array_equal(alone, v[i], equal_nan=True), (c["name"], alone, v[i])


def loud_and_quiet(sr=8000):
    loud = (tr.speech_like(5000, sr, seed=7) / np.float32(0.9)).astype(np.float32)
    quiet = (tr.speech_like(4100, sr, seed=8) * np.float32(1e-3 / 0.9)).astype(np.float32)
    other = (tr.speech_like(4507, sr, seed=9) / np.float32(0.9)).astype(np.float32)
    return [loud, quiet, other]


def normalise(waves, sr, target, gap=0, limiter=False, tp_ceiling=CEILING, ceiling=CEILING):
    packed, spans = pack(waves, gap)
    m = meter()
    y, stats, delivery = m.normalize(packed, spans, sr, target, ceiling, tp_ceiling, limiter=limiter)
    y = y.cpu().numpy()
    out = {"y": [y[b:b + n].copy() for b, n in spans], "stats": stats.cpu().numpy(), "delivery": delivery.cpu().numpy(), "whole": y,
           "packed": packed.cpu().numpy()}
    if limiter:
        g = m.last_limiter_gain.cpu().numpy()
        out.update(limiter=m.last_limiter.cpu().numpy(), g=[g[b:b + n].copy() for b, n in spans])
    else:
        out["steps"] = m.last_steps.cpu().numpy()
    return out


def test_a_quiet_utterance_between_two_loud_ones_reads_as_it_does_alone():
    """-60 dBFS between two full-scale utterances, packed tight: its true peak, its normalised and its limited output and those of
    its neighbours are bit-equal to the runs alone.  A halo read across an utterance's edge would show here first."""
    sr, waves = 8000, loud_and_quiet()
    assert abs(tr.db(float(np.abs(waves[1]).max())) + 60.0) < 0.01 and float(np.abs(waves[0]).max()) == 1.0
    rows = measure(waves, sr)
    for lim in (False, True):
        batch = normalise(waves, sr, -14.0, limiter=lim)
        for u, x in enumerate(waves):
            alone = normalise([x], sr, -14.0, limiter=lim)
            assert np.array_equal(rows[u], measure([x], sr)[0], equal_nan=True), u
            for key in ("stats", "delivery") + (("limiter",) if lim else ("steps",)):
                assert np.array_equal(batch[key][u], alone[key][0], equal_nan=True), (lim, u, key)
            assert np.array_equal(batch["y"][u].view(np.uint32), alone["y"][0].view(np.uint32)), (lim, u)
    assert rows[1][COL["true_peak"]] < 1.2e-3 and rows[0][COL["true_peak"]] > 0.9


# ---- the loudness range -------------------------------------------------------------------------------------------------------

def range_rows(energies, S=800, order=None):
    """tts_loudness_range on segment energies directly -> (rows [B, 12], zs per utterance)."""
    lib = capi.lib()
    order = list(range(len(energies))) if order is None else order
    es = [energies[i] for i in order]
    B, most = len(es), max(1, max(len(e) for e in es))
    energy = np.full((B, most), 1e30)
    for u, e in enumerate(es):
        energy[u, :len(e)] = e
    counts = np.array([len(e) * S + (S // 2 if u % 2 else 0) for u, e in enumerate(es)], dtype=np.int64)  # a partial segment changes nothing
    slots = int(-(-counts.max() // S))
    if slots > most:
        energy = np.concatenate([energy, np.full((B, slots - most), 1e30)], axis=1)
        most = slots
    begins = np.concatenate([[0], np.cumsum(counts)[:-1]])
    spans = np.ascontiguousarray(np.stack([begins, counts], axis=1).astype(np.int64))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    e_d, p_d, t_d, s_d = dev(energy), dev(np.zeros((B, most), dtype=np.float32)), dev(np.zeros(B, dtype=np.float32)), dev(spans)
    zs = torch.zeros((B, most), dtype=torch.float64, device=DEV)
    rows = torch.empty((B, len(truepeak.RANGE_COLUMNS)), dtype=torch.float64, device=DEV)
    capi.check(lib.tts_loudness_range(e_d.data_ptr(), p_d.data_ptr(), t_d.data_ptr(), int(counts.sum()), s_d.data_ptr(), B, S, most, zs.data_ptr(),
                                      rows.data_ptr(), torch.cuda.current_stream().cuda_stream), "tts_loudness_range")
    rows, zs = rows.cpu().numpy(), zs.cpu().numpy()
    back = [order.index(i) for i in range(len(energies))]
    return rows[back], [zs[u, :max(0, len(energies[i]) - 29)] for i, u in enumerate(back)]


def close(a, b, tol):
    return a == b if not (math.isfinite(a) and math.isfinite(b)) else abs(a - b) <= tol


def test_loudness_range_counts_and_order_statistics_are_exact():
    """n kept in {0, 1, 2, 10, 11, 64, 65, 129, 200} (one sweep of the wavefront is 64) and 2 100 (the kernel keeps up to 2 048
    short-term values in LDS and recomputes them beyond), with and without blocks the relative gate drops: the three counts exact; zs within its 30 additions and one division of the restatement's; low and high EXACTLY the
    restatement's order statistics of the GPU's own zs; LRA, the percentiles and the largest short-term loudness within 1e-6 LU;
    the batch reversed gives the same bits."""
    cases = tr.range_cases()
    rows, zs = range_rows([c["e"] for c in cases])
    rows_r, _ = range_rows([c["e"] for c in cases], order=list(reversed(range(len(cases)))))
    assert np.array_equal(rows, rows_r, equal_nan=True)
    for c, row, z in zip(cases, rows, zs):
        assert [int(row[COL[k]]) for k in ("short_term_blocks", "short_term_abs", "short_term_kept")] == [c["blocks"], c["kept_abs"], c["kept"]], c["name"]
        assert z.shape == c["zs"].shape and (np.abs(z - c["zs"]) <= 31 * 2.0 ** -53 * c["zs"]).all(), c["name"]
        own = tr.loudness_range(z)
        assert row[COL["lra_low_z"]] == own["low"] and row[COL["lra_high_z"]] == own["high"], (c["name"], row, own["low"], own["high"])
        for key, want in (("lra", c["lra"]), ("lra_low_lufs", c["low_lufs"]), ("lra_high_lufs", c["high_lufs"]), ("short_term_max_lufs", c["short_term_max_lufs"])):
            assert close(float(row[COL[key]]), want, 1e-6), (c["name"], key, row[COL[key]], want)
        if c["kept"] == 0:
            assert row[COL["lra"]] == 0.0 and row[COL["lra_low_lufs"]] == -math.inf and row[COL["lra_high_lufs"]] == -math.inf
    assert [int(r[COL["short_term_kept"]]) for r in rows[:9]] == [0, 1, 2, 10, 11, 64, 65, 129, 200]
    assert int(rows[11][COL["short_term_kept"]]) == 2100 and cases[11]["name"] == "kept_2100"


@pytest.mark.parametrize("i", range(len(tr.LRA_CASES)))
def test_loudness_range_of_the_analytic_cases(i):
    c = tr.lra_case(i)
    row = measure([c["x"]], 8000)[0]
    assert abs(row[COL["lra"]] - c["want"]) <= 1.0
    assert [int(row[COL[k]]) for k in ("short_term_blocks", "short_term_abs", "short_term_kept")] == [c["blocks"], c["kept_abs"], c["kept"]]
    for key, want in (("lra", c["lra"]), ("lra_low_lufs", c["low_lufs"]), ("lra_high_lufs", c["high_lufs"]), ("short_term_max_lufs", c["short_term_max_lufs"])):
        assert close(float(row[COL[key]]), want, 1e-6), (c["name"], key, row[COL[key]], want)
    e = meter().last_segments[0].cpu().numpy()[0, :len(c["e"])]
    own = tr.loudness_range(tr.short_term(e, 800))
    assert row[COL["lra_low_z"]] == own["low"] and row[COL["lra_high_z"]] == own["high"]
    print(f"{c['name']}: LRA {row[COL['lra']]:.6f} LU (restatement {c['lra']:.6f})")


# ---- the gain under the true-peak ceiling -----------------------------------------------------------------------------------

def gain_waves(sr=8000):
    return [x for _, x in tr.limiter_cases(sr, tile())] + [np.zeros(0, dtype=np.float32), np.zeros(4000, dtype=np.float32)] + loud_and_quiet(sr)


def test_the_gain_holds_the_true_peak_under_the_ceiling():
    """A target no utterance can reach under -1 dBTP.  The reading of every output is <= C, hard - by the meter and by the
    materialised path; y = x g bit for bit with g a float32; the gain and its steps are the restatement's (its chain is the
    kernel's); one float32 up the reading is over C; an utterance without a loudness keeps its bits; the loudness re-measured is
    lufs_after within 1e-5 LU."""
    sr, waves = 8000, gain_waves()
    got = normalise(waves, sr, 0.0, gap=11)
    again = loudness.LoudnessMeter(DEV).measure(*pack(got["y"]), sr).cpu().numpy()
    loudness_gain = loudness.LoudnessMeter(DEV).normalize(*pack(waves, 11), sr, 0.0, CEILING)[1].cpu().numpy()[:, LCOL["gain"]]  # g_l
    limited = 0
    for u, x in enumerate(waves):
        s, d, y = got["stats"][u], got["delivery"][u], got["y"][u]
        g = float(s[LCOL["gain"]])
        assert g == float(np.float32(g)) and np.array_equal(y.view(np.uint32), (x * np.float32(g)).view(np.uint32)), u
        assert d[0] == materialised(y, sr), (u, d)
        if not math.isfinite(s[LCOL["lufs"]]):  # no loudness: its bits, whatever its peaks
            assert g == 1.0 and got["steps"][u] == 0 and np.array_equal(y.view(np.uint32), x.view(np.uint32))
            continue
        assert d[0] <= C and d[2] <= C, (u, d)
        limited += 1
        g_l = np.float32(loudness_gain[u])
        want, steps = tr.stepped_gain(x, sr, g_l, CEILING)
        assert g <= float(g_l) and (g, int(got["steps"][u])) == (float(want), steps), (u, g, float(want), got["steps"][u], steps)
        assert materialised(x * np.nextafter(np.float32(g), np.float32(2 * g)), sr) > C or g == float(g_l), u
        assert abs(s[LCOL["lufs_after"]] - (s[LCOL["lufs"]] + 20.0 * math.log10(g))) < 1e-12
        assert abs(again[u][LCOL["lufs"]] - s[LCOL["lufs_after"]]) <= 1e-5
        if g < float(g_l):  # held by the true peak: one step up reads over C, and a step moves the reading by (1 + 2 x 61.7) u at most
            assert d[0] > C * (1 - 2.0 ** -17), (u, d[0])
    assert limited >= 6
    print("steps towards zero per utterance:", got["steps"].tolist())
    # a ceiling that does not bind leaves the loudness meter's own gain, bit for bit
    free = normalise(waves, sr, -40.0, gap=11, tp_ceiling=0.0)
    packed, spans = pack(waves, 11)
    _, plain = loudness.LoudnessMeter(DEV).normalize(packed, spans, sr, -40.0, CEILING)
    assert np.array_equal(free["stats"], plain.cpu().numpy(), equal_nan=True) and not free["steps"].any()


def test_in_place_equals_out_of_place():
    sr, waves, m = 8000, gain_waves()[:4], meter()
    packed, spans = pack(waves, 5)
    for lim in (False, True):
        out, stats, delivery = m.normalize(packed, spans, sr, -6.0, CEILING, CEILING, limiter=lim)
        assert torch.equal(packed, pack(waves, 5)[0])  # the input is left alone
        other = torch.full_like(packed, 7.0)
        out2, stats2, delivery2 = m.normalize(packed, spans, sr, -6.0, CEILING, CEILING, limiter=lim, out=other)
        inplace = packed.clone()
        out3, stats3, delivery3 = m.normalize(inplace, spans, sr, -6.0, CEILING, CEILING, limiter=lim, out=inplace)
        assert out2 is other and out3 is inplace and torch.equal(out, out3)
        for a, b in ((stats2, delivery2), (stats3, delivery3)):
            assert torch.equal(stats.nan_to_num(), a.nan_to_num()) and torch.equal(delivery.nan_to_num(), b.nan_to_num())
        for b, n in spans:
            assert torch.equal(out[b:b + n], out2[b:b + n])
        inside = torch.zeros_like(packed, dtype=torch.bool)
        for b, n in spans:
            inside[b:b + n] = True
        assert torch.equal(out[~inside], packed[~inside]) and bool((out2[~inside] == 7.0).all())  # copied into a new tensor, untouched in a given one


# ---- the limiter ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("drive", (1.0, 3.0, 6.0))
def test_limiter_against_the_restatement(drive):
    """Every utterance driven ``drive`` dB past what the pure gain can reach.  g within the rounding of its W + 1 additions and one
    division of the restatement's (which gets the GPU's own loudness); the output bit-equal to the restatement's wherever
    fl32(g) agrees, and it may disagree on at most 1e-4 of the samples; true peak and sample peak of the output <= C, hard, by
    the meter and by the materialised path; the loudness re-measured within 1e-5 LU of lufs_after; where the gain is 1 and no
    trim was needed the output is x g0 bit for bit; utterances without a loudness and of no samples keep their bits."""
    sr, waves = 8000, gain_waves()
    base = normalise(waves, sr, 0.0)  # (the loudness and the pure-gain result)
    reach = [float(s[LCOL["lufs_after"]]) for s in base["stats"]]
    W = sr // 500
    audible = [u for u, r in enumerate(reach) if math.isfinite(r)]
    total = differ = 0
    for u in audible:
        x = waves[u]
        target = reach[u] + drive
        got = normalise([x], sr, target, gap=3, limiter=True)
        s, d, row, y, g = got["stats"][0], got["delivery"][0], got["limiter"][0], got["y"][0], got["g"][0]
        ref = tr.limiter(x, sr, float(s[LCOL["lufs"]]), target, CEILING, CEILING)
        assert row[MCOL["g0"]] == float(ref["g0"]) == s[LCOL["gain"]] and row[MCOL["window"]] == W and row[MCOL["ceiling"]] == ref["C"]
        assert (np.abs(g - ref["g"]) <= (W + 2) * 2.0 ** -53 * ref["g"]).all(), u
        same = g.astype(np.float32) == ref["g"].astype(np.float32)
        total, differ = total + len(x), differ + int((~same).sum())
        assert row[MCOL["peak_before_trim"]] == ref["tp1"] and row[MCOL["trim"]] == float(ref["t"]), (u, row, ref["tp1"], ref["t"])
        assert np.array_equal(y[same].view(np.uint32), ref["y"][same].view(np.uint32)), u
        assert d[0] <= C and d[2] <= C and d[0] == materialised(y, sr) and d[2] == float(np.abs(y).max()), (u, d)
        flat = g == 1.0  # untouched by the limiter: x g0, times the trim where there was one
        untouched = x * ref["g0"] if row[MCOL["trimmed"]] == 0 else (x * ref["g0"]) * np.float32(row[MCOL["trim"]])
        assert flat.any() and np.array_equal(y[flat].view(np.uint32), untouched[flat].view(np.uint32)), u
        again = loudness.LoudnessMeter(DEV).measure(*pack([y]), sr).cpu().numpy()[0]
        assert abs(again[LCOL["lufs"]] - s[LCOL["lufs_after"]]) <= 1e-5
        # closer to the target than the one gain could bring it
        assert abs(s[LCOL["lufs_after"]] - target) < abs(reach[u] - target), (u, s[LCOL["lufs_after"]], reach[u], target)
        print(f"utterance {u} +{drive:.0f} dB: target {target:.2f}, pure gain {reach[u]:.2f}, limiter {s[LCOL['lufs_after']]:.2f} LUFS; before the trim "
              f"{row[MCOL['over_db']]:+.5f} dB re ceiling, trim {row[MCOL['trim']]:.7f}; true peak {tr.db(d[0]):.4f} dBTP")
    assert differ <= 1e-4 * total, (differ, total)
    print(f"fl32(g) differs from the restatement's on {differ} of {total} samples")
    # the whole ragged batch at once: the utterances without a loudness pass through with their bits
    batch = normalise(waves, sr, -8.0, gap=7, limiter=True)
    for u, x in enumerate(waves):
        if u not in audible:
            assert np.array_equal(batch["y"][u].view(np.uint32), x.view(np.uint32)) and batch["stats"][u][LCOL["gain"]] == 1.0
            assert len(x) == 0 or (batch["g"][u] == 1.0).all()
            assert batch["limiter"][u][MCOL["trim"]] == 1.0
    assert len(audible) >= 6 and len(audible) < len(waves)


@pytest.mark.parametrize("sr", (24000, 96000, 192000))
def test_limiter_at_other_rates(sr):
    """W = 48 at 24 kHz; F = 2 at 96 kHz; F = 1 and the widest window, 384, at 192 kHz: the restatement's gain and output there."""
    x = tr.speech_like(int(0.45 * sr) + 11, sr, seed=12)
    base = normalise([x], sr, 0.0)
    target = float(base["stats"][0][LCOL["lufs_after"]]) + 4.0
    got = normalise([x], sr, target, gap=2, limiter=True)
    s, d, row, y, g = got["stats"][0], got["delivery"][0], got["limiter"][0], got["y"][0], got["g"][0]
    ref = tr.limiter(x, sr, float(s[LCOL["lufs"]]), target, CEILING, CEILING)
    W = sr // 500
    assert row[MCOL["window"]] == W and (np.abs(g - ref["g"]) <= (W + 2) * 2.0 ** -53 * ref["g"]).all() and g.min() < 0.8
    same = g.astype(np.float32) == ref["g"].astype(np.float32)
    assert (~same).sum() <= max(1, 1e-4 * len(x)) and np.array_equal(y[same].view(np.uint32), ref["y"][same].view(np.uint32))
    assert d[0] <= C and d[2] <= C and d[0] == materialised(y, sr)


# ---- the interface ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tts(tmp_path_factory):
    """Fixture weights in the bf16 configuration: a 16-bit configuration synthesises an utterance bit for bit whatever the batch."""
    models = tmp_path_factory.mktemp("truepeak_models") / "Models"
    interface.write_fixture_checkpoints(str(models), n_lang=20)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(interface, "MODELS_DIR", str(models))
        mp.setenv("TOUCAN_PRECISION", "bf16")
        mp.delenv("TOUCAN_PY_SEQUENCER", raising=False)
        yield interface.ToucanTTSInterface(device=DEV, tts_model_path="Meta", faster_vocoder=True)


PHONES = ["~həlˈoʊ~#", "~wˈɜːld tˈu~#", "~wˈʌns əpˈɑːn ɐ mˈɪdnaɪt~#"]


def gold(tts, phones, frames=6, seed=3):
    L = int(tts.text2phone.string_to_tensor(phones, input_phonemes=True).shape[0])
    z = torch.randn(80, frames * L, generator=torch.Generator().manual_seed(seed)) * 0.8
    return torch.full((L,), frames, dtype=torch.long), z


def read(waves):
    """The meter's rows of the 24 kHz waves."""
    return measure([w.float().cpu().numpy() for w in waves], 24000)


def test_interface_defaults_are_the_loudness_call_as_it_was(tts):
    d, z = gold(tts, PHONES[2])
    kw = dict(input_is_phones=True, durations=d, z_noise=z, loudness=-23.0)
    tts.last_delivery = None
    before = capi.CALLS
    plain = tts(PHONES[2], **kw)
    calls = capi.CALLS - before
    rows = tts.last_loudness.clone()
    before = capi.CALLS
    same = tts(PHONES[2], true_peak_ceiling=None, limiter=False, **kw)
    assert capi.CALLS - before == calls and torch.equal(same, plain) and torch.equal(tts.last_loudness, rows) and tts.last_delivery is None
    held = tts(PHONES[2], true_peak_ceiling=-1.0, **kw)
    assert tts.last_delivery.shape == (1, 8) and tts.last_delivery.dtype == torch.float64 and tts.last_delivery.is_cuda
    row = read([held])[0]
    assert np.array_equal(tts.last_delivery.cpu().numpy()[0], row[:8], equal_nan=True)
    assert row[COL["true_peak_dbtp"]] <= -1.0 and math.isfinite(rows[0, 0].item()), "the fixture voice is expected to be audible"


def test_interface_limiter_gets_closer_to_a_target_the_gain_cannot_reach(tts):
    """Batch, through the 24 kHz stage of ``sample_rate=48000, pcm16=True``, grid and file: with a target 4 dB past what the pure
    gain reaches under -1 dBTP, the pure gain ends at the ceiling and below the target, the limiter closer to the target, both
    with a true peak <= -1 dBTP by the meter's reading of the 24 kHz result."""
    dz = [gold(tts, p, seed=s) for s, p in enumerate(PHONES)]
    kw = dict(durations=[d for d, _ in dz], z_noise=[z for _, z in dz])
    tts.synthesize_batch(PHONES, loudness=0.0, true_peak_ceiling=-1.0, **kw)
    reach = tts.last_loudness.cpu().numpy()[:, LCOL["lufs_after"]]
    assert np.isfinite(reach).all(), "the fixture voice is expected to be audible"
    target = float(reach.max()) + 4.0
    gain = tts.synthesize_batch(PHONES, loudness=target, true_peak_ceiling=-1.0, **kw)
    gain_rows, gain_delivery = tts.last_loudness.cpu().numpy(), tts.last_delivery.cpu().numpy()
    lim = tts.synthesize_batch(PHONES, loudness=target, true_peak_ceiling=-1.0, limiter=True, **kw)
    lim_rows, lim_delivery = tts.last_loudness.cpu().numpy(), tts.last_delivery.cpu().numpy()
    for waves, delivery in ((gain, gain_delivery), (lim, lim_delivery)):
        now = read(waves)
        assert np.array_equal(now[:, :8], delivery, equal_nan=True) and (now[:, COL["true_peak_dbtp"]] <= -1.0).all() and (now[:, COL["sample_peak"]] <= C).all()
    again = loudness.LoudnessMeter(DEV).measure(*pack([w.cpu().numpy() for w in lim]), 24000).cpu().numpy()
    for u in range(len(PHONES)):
        assert abs(gain_rows[u, LCOL["lufs_after"]] - reach[u]) < 1e-9 and reach[u] < target - 3.9
        assert abs(lim_rows[u, LCOL["lufs_after"]] - target) < abs(gain_rows[u, LCOL["lufs_after"]] - target), u
        assert abs(again[u, LCOL["lufs"]] - lim_rows[u, LCOL["lufs_after"]]) <= 1e-5
    print("target", target, "pure gain", gain_rows[:, LCOL["lufs_after"]].tolist(), "limiter", lim_rows[:, LCOL["lufs_after"]].tolist(),
          "dBTP", lim_delivery[:, 1].tolist())
    # 48 kHz PCM16: the resampler on the limited 24 kHz wave, the statistics those of that stage
    got = tts.synthesize_batch(PHONES, sample_rate=48000, pcm16=True, loudness=target, true_peak_ceiling=-1.0, limiter=True, **kw)
    assert np.array_equal(tts.last_delivery.cpu().numpy(), lim_delivery, equal_nan=True)
    packed, spans = pack([w.cpu().numpy() for w in lim])
    want, out_spans = resampler().resample(packed, spans, 24000, 48000, pcm16=True)
    for g, (b, n) in zip(got, out_spans):
        assert g.dtype == torch.int16 and torch.equal(g, want[b:b + n])
    # forward, grid and file give the batch's rows
    one = tts(PHONES[1], input_is_phones=True, durations=dz[1][0], z_noise=dz[1][1], loudness=target, true_peak_ceiling=-1.0, limiter=True)
    assert torch.equal(one, lim[1]) and np.array_equal(tts.last_delivery.cpu().numpy()[0], lim_delivery[1], equal_nan=True)
    grid = tts.synthesize_grid(PHONES[2], energy_variance_scales=(1.0, 2.5), durations=dz[2][0], z_noise=[dz[2][1]] * 2, loudness=target, limiter=True)
    assert tts.last_delivery.shape == (2, 8) and torch.equal(torch.stack([v["delivery"] for v in grid]), tts.last_delivery)
    assert torch.equal(grid[0]["wave"], lim[2]) and (tts.last_delivery[:, 1] <= -1.0).all()
    plain = tts.synthesize_grid(PHONES[2], energy_variance_scales=(1.0,), durations=dz[2][0], z_noise=[dz[2][1]], loudness=target)
    assert "delivery" not in plain[0]


def test_interface_read_to_file_and_ensemble(tts, tmp_path):
    out = tmp_path / "delivery.wav"
    texts = [PHONES[0], "", PHONES[2]]
    d = [gold(tts, PHONES[0])[0], None, gold(tts, PHONES[2])[0]]
    tts.read_to_file(texts, str(out), silent=True, input_is_phones=True, dur_list=d, loudness=-16.0, true_peak_ceiling=-2.0)
    rows = tts.last_delivery.cpu().numpy()
    assert rows.shape == (2, 8) and tts.last_loudness.shape == (2, 8) and (rows[:, 1] <= -2.0).all()
    d0, z0 = gold(tts, PHONES[0])
    voices = dict(utterance_embeddings=[tts.default_utterance_embedding, tts.default_utterance_embedding * 0.5], durations=d0, z_noise=[z0] * 2)
    ens = tts.synthesize_ensemble(PHONES[0], loudness=0.0, true_peak_ceiling=-3.0, **voices)
    row = read([ens])[0]
    assert tts.last_delivery.shape == (1, 8) and row[COL["true_peak_dbtp"]] <= -3.0 and row[COL["true_peak_dbtp"]] > -3.001
    with pytest.raises(ValueError, match="true-peak ceiling"):
        next(tts.stream(PHONES[0], input_is_phones=True, loudness=-23.0, limiter=True))
