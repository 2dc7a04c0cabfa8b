"""The sample-rate converter without a GPU: the table against what style.resample_sinc applies, the output lengths, the streamer's
bookkeeping on a numpy stand-in for the kernel, float2pcm on the probe, the keyword errors of the interface, and the binding of
include/toucan_resample.h."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import build, capi, interface, resample, style
from tests import resample_ref as rr

HERE = os.path.dirname(os.path.abspath(__file__))
TILE = 1024
ALL = sorted(rr.RATIOS)


@pytest.mark.parametrize("sr_in,sr_out", ALL)
def test_kernel_table_is_what_resample_sinc_applies(sr_in, sr_out):
    """Unit impulses through style.resample_sinc read its coefficients out one by one: an impulse at q puts k[p][q + w - i orig]
    at output i new + p.  The impulses q = w .. w + orig - 1 reach every tap; each equals the table's entry after the cast."""
    orig, new, w, tab = resample.kernel_table(sr_in, sr_out)
    assert (orig, new, tab.shape[1]) == rr.RATIOS[(sr_in, sr_out)] and tab.shape == (new, 2 * w + orig) and tab.dtype == np.float32
    ro, rn, rw, rk = rr.table(sr_in, sr_out)
    assert (ro, rn, rw) == (orig, new, w) and np.array_equal(rk.astype(np.float32), tab)
    K, n = tab.shape[1], 2 * w + 3 * orig
    seen = np.zeros(K, dtype=bool)
    for q in range(w, w + orig):
        x = np.zeros(n)
        x[q] = 1.0
        y = style.resample_sinc(x, sr_in, sr_out)
        for i in range((q + w) // orig + 1):
            j = q + w - i * orig
            assert np.array_equal(y[i * new:(i + 1) * new], tab[:, j]), (q, i)
            seen[j] = True
    assert seen.all()


def test_equal_rates_are_the_identity_table():
    assert [v if np.isscalar(v) else v.tolist() for v in resample.kernel_table(24000, 24000)] == [1, 1, 0, [[1.0]]]
    assert resample.out_length(777, 16000, 16000) == 777


@pytest.mark.parametrize("sr_in,sr_out", ALL)
def test_out_length(sr_in, sr_out):
    orig, new, K = rr.RATIOS[(sr_in, sr_out)]
    for n, _ in rr.lengths(sr_in, sr_out, TILE) + [(0, 0), (orig, new), (245760, 0)]:
        want = (new * n + orig - 1) // orig
        assert resample.out_length(n, sr_in, sr_out) == rr.out_length(n, sr_in, sr_out) == want
        if 0 < n < 4000:
            assert len(style.resample_sinc(np.zeros(n), sr_in, sr_out)) == want
    # every exact tile count is met by the utterance lengths() pairs it with
    for n, count in rr.lengths(sr_in, sr_out, TILE)[4:7]:
        assert count <= resample.out_length(n, sr_in, sr_out) and (n == 0 or resample.out_length(n - 1, sr_in, sr_out) < count)
    assert [c for _, c in rr.lengths(sr_in, sr_out, TILE)[4:7]] == [TILE - 1, TILE, TILE + 1]
    assert rr.lengths(sr_in, sr_out, TILE)[-1][1] > 2 * TILE
    assert orig == 1 or rr.lengths(sr_in, sr_out, TILE)[3][0] % orig != 0


def window_outputs(buf, pos0, out_first, out_count, sr_in, sr_out):
    """The entry point's definition in numpy float64: outputs of the utterance whose samples pos0 ... the buffer holds."""
    orig, new, w, kern = rr.table(sr_in, sr_out)
    K, out = kern.shape[1], np.empty(out_count)
    for lo in range(0, out_count, 32768):
        m = out_first + np.arange(lo, min(out_count, lo + 32768))
        idx = (m // new * orig - w - pos0)[:, None] + np.arange(K)[None, :]
        vals = np.where((idx >= 0) & (idx < len(buf)), buf[np.clip(idx, 0, len(buf) - 1)], 0.0)
        out[lo:lo + len(m)] = (kern[m % new] * vals).sum(axis=1)
    return out


def test_window_stand_in_is_the_restatement():
    x = rr.noise(1000).astype(np.float64)
    got = window_outputs(x, 0, 0, rr.out_length(1000, 24000, 44100), 24000, 44100)
    assert np.abs(got - rr.resample(x, 24000, 44100)).max() < 1e-14


@pytest.mark.parametrize("sr_in,sr_out,piece", [(a, b, p) for a, b in ((24000, 44100), (24000, 16000), (44100, 16000), (24000, 48000))
                                               for p in ("1", "orig-1", "orig+1", "7919", "196608") if p != "196608" or (a, b) == (24000, 44100)])
def test_streamer_bookkeeping(sr_in, sr_out, piece):
    """Whatever the piece length, the launches ask for index ranges that tile 0 .. ceil(new n / orig) exactly once and in order, every
    pushed range has all its K samples, and the pieces joined equal the whole converted at once (the same float64 sums: exact)."""
    orig, new, K = rr.RATIOS[(sr_in, sr_out)]
    w = (K - orig) // 2
    L = max(1, {"1": 1, "orig-1": orig - 1, "orig+1": orig + 1, "7919": 7919, "196608": 196608}[piece])
    n = {"1": 2 * K + 7, "7919": 3 * 7919 + 5, "196608": 196608 + 7919 + 1}.get(piece, 10 * L + 3 + 4 * K)
    x = rr.noise(n, seed=5).astype(np.float64)
    asked = []

    def launch(buf, pos0, out_first, out_count):
        asked.append((out_first, out_count, pos0, len(buf)))
        return window_outputs(buf, pos0, out_first, out_count, sr_in, sr_out)

    st = resample.Streamer(launch, orig, new, w, np.concatenate, lambda: np.empty(0))
    outs = []
    for lo in range(0, n, L):
        launches, received = len(asked), min(n, lo + L)
        outs.append(st.push(x[lo:lo + L]))
        assert len(asked) - launches == (1 if len(outs[-1]) else 0)
        if len(asked) > launches:
            first, count, pos0, held = asked[-1]
            assert pos0 + held == received
            # the last output pushed reads no sample that has not arrived
            assert (first + count - 1) // new * orig + K - 1 - w <= received - 1
        assert st.tail_pos + len(st.tail) == received and len(st.tail) <= K
    pushed = len(asked)
    outs.append(st.finish())
    total = rr.out_length(n, sr_in, sr_out)
    at = 0
    for k, (first, count, pos0, held) in enumerate(asked):
        assert first == at and count > 0
        assert pos0 <= max(0, first // new * orig - w), "a sample the range reads was dropped from the tail"
        at += count
    assert at == total and len(asked) - pushed <= 1
    # exactly the complete outputs were pushed: the next block's samples had not all arrived
    before_finish = sum(c for _, c, _, _ in asked[:pushed])
    assert before_finish % new == 0 and (before_finish // new + 1) * orig + w > n
    whole = window_outputs(x, 0, 0, total, sr_in, sr_out)
    assert np.array_equal(np.concatenate(outs), whole)
    with pytest.raises(AssertionError):
        st.push(x[:1])


def test_float2pcm_semantics_on_the_probe():
    """Scale by 32768, saturate to [-32768, 32767], drop the fraction toward zero - no rounding."""
    p = rr.pcm_probe()
    got = interface.float2pcm(p)
    assert got.dtype == np.int16 and np.array_equal(got, rr.float2pcm_int16(p))
    want = {1.0: 32767, -1.0: -32768, 0.5 / 32768: 0, -0.5 / 32768: 0, 1.5 / 32768: 1, -1.5 / 32768: -1, 1.25: 32767, -1.25: -32768,
            3.0e4: 32767, -3.0e4: -32768, 100.9 / 32768: 100, -100.9 / 32768: -100, 32766.5 / 32768: 32766, 32767.5 / 32768: 32767,
            -32767.5 / 32768: -32767}
    for v, q in want.items():
        assert int(interface.float2pcm(np.array([v], dtype=np.float32))[0]) == q, v
    assert int(got[7]) == 32767  # the largest float below 1: 32767.998 is cut, not rounded up and saturated
    exact = np.trunc(np.clip(p.astype(np.float64) * 32768.0, -32768, 32767)).astype(np.int16)
    assert np.array_equal(got, exact)


def test_ratio_past_the_limit_is_refused_and_names_the_limit():
    with pytest.raises(ValueError, match=str(capi.RESAMPLE_MAX_FACTOR)):
        resample.kernel_table(24000, 44101)
    with pytest.raises(ValueError, match="TTS_RESAMPLE_MAX_FACTOR"):
        resample.out_length(10, 24000, 44101)
    for bad in (0, -16000, 22050.5, True):
        with pytest.raises(ValueError):
            resample.ratio(24000, bad)
    for sr_in, sr_out in ALL + [(48000, 16000), (24000, 11025), (8000, 44100), (1024, 1)]:
        assert max(resample.ratio(sr_in, sr_out)) <= capi.RESAMPLE_MAX_FACTOR


def test_interface_keyword_errors():
    """increased_compatibility_mode with sample_rate, distributed=True with either keyword, and a rate past the limit raise
    ValueError before anything is synthesised (the object has no engines)."""
    tts = object.__new__(interface.ToucanTTSInterface)
    with pytest.raises(ValueError, match="increased_compatibility_mode"):
        tts.read_to_file(["a"], "x.wav", increased_compatibility_mode=True, sample_rate=16000)
    with pytest.raises(ValueError, match="distributed"):
        tts.synthesize_batch(["a"], distributed=True, sample_rate=16000)
    with pytest.raises(ValueError, match="distributed"):
        tts.synthesize_batch(["a"], distributed=True, pcm16=True)
    for call in (lambda: tts.forward("a", sample_rate=44101), lambda: tts.synthesize_batch(["a"], sample_rate=44101),
                 lambda: tts.synthesize_ensemble("a", [None], sample_rate=44101), lambda: next(tts.stream("a", sample_rate=44101)),
                 lambda: tts.read_to_file(["a"], "x.wav", sample_rate=44101)):
        with pytest.raises(ValueError, match="1024"):
            call()
    assert tts._check_output_format(None, False) is False and tts._check_output_format(24000, False) is False
    assert tts._check_output_format(24000, True) is True and tts._check_output_format(16000, False) is True


def test_resample_header_binding_and_library_agree():
    """include/toucan_resample.h, capi.RESAMPLE_PROTOTYPES and the symbols libtoucan_hip.so exports are the same set, with the
    constants and the span layout the binding mirrors; the entry refuses a ratio past the limit and names the limit."""
    root = os.path.dirname(HERE)
    raw = open(os.path.join(root, "include", "toucan_resample.h"), encoding="utf-8").read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(tts_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.RESAMPLE_PROTOTYPES) == ["tts_resample", "tts_resample_tile_outputs"]
    for other in (capi.PROTOTYPES, capi.ALIGN_PROTOTYPES, capi.SCORE_PROTOTYPES, capi.GAN_PROTOTYPES, capi.PITCH_PROTOTYPES, capi.TRAIN_PROTOTYPES):
        assert not set(declared) & set(other)
    macros = {k: int(v) for k, v in re.findall(r"#define\s+(TTS_RESAMPLE_[A-Z_]+)\s+(\d+)", text)}
    assert macros == {"TTS_RESAMPLE_MAX_FACTOR": capi.RESAMPLE_MAX_FACTOR, "TTS_RESAMPLE_LDS_TABLE_BYTES": capi.RESAMPLE_LDS_TABLE_BYTES}
    fields = re.findall(r"int64_t\s+(\w+);", re.search(r"typedef struct TtsResampleSpan \{(.*?)\}", text, flags=re.S).group(1))
    assert fields == [f for f, _ in capi.TtsResampleSpan._fields_] and ctypes.sizeof(capi.TtsResampleSpan) == 48
    args = re.search(r"\bint\s+tts_resample\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    assert len(args.split(",")) == len(capi.RESAMPLE_PROTOTYPES["tts_resample"][1])
    assert "resample.hip" in build.SOURCES
    build.build()
    handle = capi.lib()
    assert isinstance(handle, ctypes.CDLL)
    for n in declared:
        fn = getattr(handle, n)
        assert fn.argtypes == capi.RESAMPLE_PROTOTYPES[n][1] and fn.restype == capi.RESAMPLE_PROTOTYPES[n][0], n
    assert handle.tts_abi_version() == 15
    assert handle.tts_resample_tile_outputs() == TILE
    # argument errors are found before anything touches a device
    assert handle.tts_resample(None, None, None, 1, 10, 24000, 44101, 7, 0, None, None) == -1
    assert "TTS_RESAMPLE_MAX_FACTOR = 1024" in handle.tts_last_error().decode()
    assert handle.tts_resample(None, None, None, 1, 10, 6, 4, 7, 0, None, None) == -1 and "coprime" in handle.tts_last_error().decode()
    # the largest table in use is past the LDS regime, the others inside: both regimes are in the ratio list
    sizes = {r: 4 * new * K for r, (orig, new, K) in rr.RATIOS.items()}
    assert sizes[(44100, 16000)] == 304000 > capi.RESAMPLE_LDS_TABLE_BYTES and sizes[(24000, 22050)] > capi.RESAMPLE_LDS_TABLE_BYTES
    assert sizes[(24000, 44100)] == 55272 <= capi.RESAMPLE_LDS_TABLE_BYTES and sizes[(24000, 48000)] == 120
    assert math.gcd(441, 160) == 1
