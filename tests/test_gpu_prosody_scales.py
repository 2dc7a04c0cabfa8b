"""Per-utterance prosody scales on a real MI355X (include/toucan_prosody.h):
 (1) tts_prosody_control_v against the scalar tts_prosody_control run on every utterance alone - bit for bit, NaNs included;
 (2) tts_prosody_stats against the float64 restatement (tests/prosody_ref.py), and batch == alone bit for bit;
 (3) the stage entry (native.NativePipeline.forward with per-utterance lists) against every utterance run alone with its scalars,
     against the Python sequencer (engine.py), and both sequencers' statistics against the restatement;
 (4) the scalar call still takes the scalar entry and equals the same values given as lists;
 (5) synthesize_grid against forward() per variant, and the realised variance ratio of its statistics.
fp32 tolerances of a batch against an utterance alone (mel max-abs 5e-4 / mean-abs 1e-4, waveform max-abs 5e-4): the fp32 figures of
tests/test_gpu_native_pipeline.py; the 16-bit configurations are bit-identical whatever the batch."""
import numpy as np
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import capi, engine, fixture_weights as fw, native, prosody, synthetic as syn
from ims_toucan_prosody_variance_amd.phonemes import phones_to_features
from ims_toucan_prosody_variance_amd.ragged import Ragged
from tests import prosody_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_LANG = 20
SCALES = [(1.0, 1.3, 1.0, 0.7), (0.9, 1.0, 0.8, 1.0), (1.2, 1.5, 1.0, 1.3), (1.0, 1.0, 1.0, 1.0)]  # (duration, pitch, energy, pause)


def _bits(t):
    return t.view(torch.int32)


# ---- (1), (2): the kernels ---------------------------------------------------------------------------------------------------------
LENGTHS = [1, 7, 257, 1000]  # one row; less than a sweep; a sweep of 256 and a tail of one; several sweeps and a tail
UNVOICED = 2                 # this utterance has no voiced phoneme and a pitch scale of 1.5: the mean of nothing, NaN


@pytest.fixture(scope="module")
def kernel_batch():
    rng = np.random.default_rng(23)
    R = sum(LENGTHS)
    text = np.zeros((R, 62), dtype=np.float32)
    text[:, ref.F_VOICED] = rng.random(R) < 0.6
    text[:, ref.F_PHONEME] = rng.random(R) < 0.8
    text[:, ref.F_WORD_BOUNDARY] = rng.random(R) < 0.15
    text[:, ref.F_SILENCE] = rng.random(R) < 0.2
    text[0, ref.F_VOICED] = 1  # (the one-row utterance keeps its pitch: its mean is itself)
    b = sum(LENGTHS[:UNVOICED])
    text[b:b + LENGTHS[UNVOICED], ref.F_VOICED] = 0
    pitch = (0.3 + 0.5 * rng.standard_normal(R)).astype(np.float32)  # (spread over the mean: the clamp at 0 bites)
    energy = (0.5 + 0.4 * rng.standard_normal(R)).astype(np.float32)
    dur = rng.integers(0, 13, R).astype(np.int32)
    return dict(text=text, pitch=pitch, energy=energy, dur=dur)


def _dev(kb, sl=slice(None)):
    return tuple(torch.from_numpy(kb[k][sl].copy()).to(DEV) for k in ("text", "pitch", "energy", "dur"))


def _stats(ops, p, e, d, rag):
    return ops.prosody_stats(p, e, d, rag, torch.full((rag.n_seq, capi.PROSODY_STATS), -7.0, device=DEV))


def test_control_v_equals_the_scalar_kernel_on_every_utterance_alone(kernel_batch):
    ops = engine.Ops(DEV)
    rag = Ragged(LENGTHS, DEV)
    text, p, e, d = _dev(kernel_batch)
    ops.prosody_control_v(text, p, e, d, rag, torch.tensor(SCALES, dtype=torch.float32, device=DEV))
    # scales None = the overrides alone = the scalar kernel with every scale 1
    t0, p0, e0, d0 = _dev(kernel_batch)
    ops.prosody_control_v(t0, p0, e0, d0, rag, None)
    t1, p1, e1, d1 = _dev(kernel_batch)
    ops.prosody_control(t1, p1, e1, d1, rag, 1.0, 1.0, 1.0, 1.0)
    assert torch.equal(d0, d1) and torch.equal(_bits(p0), _bits(p1)) and torch.equal(_bits(e0), _bits(e1))
    # overrides, then scales: the bits of the one call with scales (what the stage entry relies on)
    ops.prosody_control_v(t0, p0, e0, d0, rag, torch.tensor(SCALES, dtype=torch.float32, device=DEV))
    assert torch.equal(d0, d) and torch.equal(_bits(p0), _bits(p)) and torch.equal(_bits(e0), _bits(e))
    for u, (b, n) in enumerate(zip(rag.begins, rag.lengths)):
        tu, pu, eu, du = _dev(kernel_batch, slice(b, b + n))
        ops.prosody_control(tu, pu, eu, du, Ragged([n], DEV), *SCALES[u])
        assert torch.equal(d[b:b + n], du), u
        assert torch.equal(_bits(p[b:b + n]), _bits(pu)), u
        assert torch.equal(_bits(e[b:b + n]), _bits(eu)), u
        if u == UNVOICED:
            assert torch.isnan(pu).all()
        else:
            assert torch.isfinite(pu).all() and torch.isfinite(eu).all()
    # and the definition: durations equal, pitch / energy to fp32 rounding ((n + 6) eps (1 + |s|) max|v|: tests/test_prosody_scales_cpu.py)
    gp, ge, gd = ref.control(kernel_batch["text"], kernel_batch["pitch"], kernel_batch["energy"], kernel_batch["dur"], LENGTHS, np.float32(SCALES))
    assert np.array_equal(d.cpu().numpy(), gd)
    for got, want, raw, col in ((p, gp, kernel_batch["pitch"], 1), (e, ge, kernel_batch["energy"], 2)):
        got = got.cpu().numpy().astype(np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        for u, (b, n) in enumerate(zip(rag.begins, rag.lengths)):
            if u == UNVOICED and col == 1:
                continue
            tol = (n + 6) * 2.0 ** -23 * (1 + abs(SCALES[u][col])) * float(np.abs(raw[b:b + n]).max())
            assert np.abs(got[b:b + n] - want[b:b + n]).max() <= tol, (u, col)


def test_stats_match_the_restatement_and_do_not_depend_on_the_batch(kernel_batch):
    ops = engine.Ops(DEV)
    rag = Ragged(LENGTHS, DEV)
    text, p, e, d = _dev(kernel_batch)
    for scales in (None, torch.tensor(SCALES, dtype=torch.float32, device=DEV)):  # after the overrides; after the scales (one NaN utterance)
        ops.prosody_control_v(text, p, e, d, rag, scales)
        got = _stats(ops, p, e, d, rag)
        ph, eh, dh = p.cpu().numpy(), e.cpu().numpy(), d.cpu().numpy()
        want = ref.stats(ph, eh, dh, LENGTHS)
        print("stats", "after the overrides" if scales is None else "after the scales", "\n", got.cpu().numpy(), "\n", want)
        ref.assert_stats_match(got.cpu().numpy(), want)
        assert bool(np.isnan(want[UNVOICED, 1])) == (scales is not None)
        for u, (b, n) in enumerate(zip(rag.begins, rag.lengths)):
            alone = _stats(ops, p[b:b + n].clone(), e[b:b + n].clone(), d[b:b + n].clone(), Ragged([n], DEV))
            assert torch.equal(_bits(alone[0]), _bits(got[u])), u


# ---- (3): the stage entry and the Python sequencer -----------------------------------------------------------------------------------
US, LS = [300, 301, 302, 303], [7, 20, 20, 7]
LISTS = {name: [s[k] for s in SCALES] for k, name in enumerate(prosody.KNOBS)}


def _stage_inputs():
    feats = [torch.from_numpy(syn.utterance_features(u, L)) for u, L in zip(US, LS)]
    embs = torch.from_numpy(np.stack([syn.utterance_embedding(u) for u in US]))
    zs = [torch.from_numpy(syn.postflow_noise(u, 512)) for u in US]
    return feats, embs, [syn.LANG_EN] * 4, zs


@pytest.fixture(scope="module", params=["bf16", "f32"])
def stage(request):
    precision = request.param
    ac_sd, voc_sd = fw.acoustic_state_dict(), fw.bigvgan_state_dict()
    pipe = native.NativePipeline(ac_sd, voc_sd, "bigvgan", DEV, precision=precision)
    feats, embs, langs, zs = _stage_inputs()
    out = pipe.forward(feats, embs, langs, z_noise=zs, **LISTS)
    return dict(precision=precision, pipe=pipe, ac_sd=ac_sd, voc_sd=voc_sd, out=out, wav=out["wav"])  # (every forward() returns tensors of its own)


def test_stage_batch_equals_every_utterance_alone_with_its_scalars(stage):
    pipe, out, wav = stage["pipe"], stage["out"], stage["wav"]
    feats, embs, langs, zs = _stage_inputs()
    assert "prosody_stats" in out
    for u in range(4):
        one = pipe.forward([feats[u]], embs[u:u + 1], [langs[u]], z_noise=[zs[u]], **{name: LISTS[name][u] for name in prosody.KNOBS})
        assert "prosody_stats" not in one  # (the scalar entry)
        assert torch.equal(one["durations"][0], out["durations"][u]), u
        assert torch.equal(_bits(one["pitch"][0]), _bits(out["pitch"][u])), u
        assert torch.equal(_bits(one["energy"][0]), _bits(out["energy"][u])), u
        b, n = out["wav_spans"][u]
        b1, n1 = one["wav_spans"][0]
        assert n == n1 and one["mel"][0].shape == out["mel"][u].shape
        if stage["precision"] == "bf16":  # the 16-bit contract: bit for bit whatever the batch
            assert torch.equal(one["mel"][0], out["mel"][u]), u
            assert torch.equal(one["wav"][b1:b1 + n1], wav[b:b + n]), u
        else:
            err = (one["mel"][0] - out["mel"][u]).abs()
            print(f"fp32, utterance {u}: mel max {float(err.max()):.3e} mean {float(err.mean()):.3e}, "
                  f"wav max {float((one['wav'][b1:b1 + n1] - wav[b:b + n]).abs().max()):.3e}")
            assert float(err.max()) < 5e-4 and float(err.mean()) < 1e-4, u
            assert float((one["wav"][b1:b1 + n1] - wav[b:b + n]).abs().max()) < 5e-4, u


def test_python_sequencer_equals_the_stage_entry_and_both_report_the_statistics(stage):
    pipe, out, wav, precision = stage["pipe"], stage["out"], stage["wav"], stage["precision"]
    feats, embs, langs, zs = _stage_inputs()
    ac = engine.AcousticEngine(stage["ac_sd"], DEV, precision=precision)
    voc = engine.VocoderEngine(stage["voc_sd"], "bigvgan", DEV, precision=precision)
    py = ac.forward(feats, embs, langs, z_noise=zs, **LISTS)
    wpy, rw = voc.forward(py["mel_packed"], py["rag_mel"])
    for u in range(4):
        assert torch.equal(py["durations"][u], out["durations"][u]), u
        assert torch.equal(_bits(py["pitch"][u]), _bits(out["pitch"][u])), u
        assert torch.equal(_bits(py["energy"][u]), _bits(out["energy"][u])), u
        assert torch.equal(py["mel"][u], out["mel"][u]), u
        b, n = out["wav_spans"][u]
        assert (b, n) == (rw.begins[u], rw.lengths[u])
        assert torch.equal(wpy[b:b + n], wav[b:b + n]), u
    for a, b in zip(py["prosody_stats"], out["prosody_stats"]):
        assert a.dtype == b.dtype == np.float32 and a.shape == b.shape == (4, capi.PROSODY_STATS)
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    # the restatement: "before" from a pass without scales (its pitch / energy / durations are the overridden predictions),
    # "after" from the batch's own result
    plain = pipe.forward(feats, embs, langs, run_postflow=False, vocode=False)
    cat = lambda o, k: torch.cat(o[k]).cpu().numpy()
    before, after = out["prosody_stats"]
    ref.assert_stats_match(before, ref.stats(cat(plain, "pitch"), cat(plain, "energy"), cat(plain, "durations"), LS))
    ref.assert_stats_match(after, ref.stats(cat(out, "pitch"), cat(out, "energy"), cat(out, "durations"), LS))
    assert np.array_equal(after[:, 7], LS) and np.array_equal(after[3], before[3])  # utterance 3: every scale 1
    frames = [int(d.sum()) for d in out["durations"]]
    assert np.array_equal(after[:, 6], frames)


# ---- (4), (5): the interface -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models_dir(tmp_path_factory):
    from ims_toucan_prosody_variance_amd import interface
    d = tmp_path_factory.mktemp("Models")
    interface.write_fixture_checkpoints(str(d), n_lang=N_LANG)
    return str(d)


def _tts(models_dir, monkeypatch, precision):
    from ims_toucan_prosody_variance_amd import interface
    monkeypatch.setattr(interface, "MODELS_DIR", models_dir)
    monkeypatch.setenv("TOUCAN_PRECISION", precision)
    monkeypatch.delenv("TOUCAN_PY_SEQUENCER", raising=False)
    tts = interface.ToucanTTSInterface(device="cuda", tts_model_path="Meta", faster_vocoder=True)
    tts.set_language("en")
    assert tts.pipe is not None
    return tts


class CountingLib:
    """The bound library with a count of the calls per entry."""

    def __init__(self, lib):
        self._lib, self.counts = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*args):
            self.counts[name] = self.counts.get(name, 0) + 1
            return fn(*args)
        return counted


PHONES_20 = "~wˈʌns əpˈɑːn mˈɪdnaɪt~#"
PHONES_13 = "~həlˈoʊ wˈɜːld~#"


def test_scalar_call_keeps_the_scalar_entry_and_equals_the_lists(models_dir, monkeypatch):
    tts = _tts(models_dir, monkeypatch, "f32")
    texts = [PHONES_20, PHONES_13, PHONES_20]
    zs = [torch.from_numpy(syn.postflow_noise(40 + i, 512)) for i in range(3)]
    values = dict(duration_scaling_factor=0.9, pitch_variance_scale=1.3, energy_variance_scale=0.8, pause_duration_scaling_factor=1.2)
    tts.pipe.lib = spy = CountingLib(tts.pipe.lib)
    scalar = tts.synthesize_batch(texts, z_noise=zs, **values)
    assert spy.counts.get("tts_control_and_regulate") == 1 and "tts_control_and_regulate_v" not in spy.counts
    assert "tts_copy_prosody_stats" not in spy.counts and tts.last_prosody_stats is None
    d_scalar = [d.clone() for d in tts.last_durations]
    spy.counts.clear()
    listed = tts.synthesize_batch(texts, z_noise=zs, **{k: [v] * 3 for k, v in values.items()})
    assert spy.counts.get("tts_control_and_regulate_v") == 1 and "tts_control_and_regulate" not in spy.counts
    before, after = tts.last_prosody_stats
    assert before.shape == after.shape == (3, 8)
    for a, b, da, db in zip(scalar, listed, d_scalar, tts.last_durations):
        assert torch.equal(da, db) and torch.equal(a, b)
    # one list among scalars: the scalars are broadcast
    mixed = tts.synthesize_batch(texts, z_noise=zs, **dict(values, pitch_variance_scale=[1.3] * 3))
    assert all(torch.equal(a, b) for a, b in zip(scalar, mixed))


def _grid_gold(L, voiced):
    """Gold pitch of the grid sentence, chosen on the CPU with the restatement: every voiced phoneme within [0.55, 1.45] around a mean
    near 1, so that the pitch scale 1.5 clamps no entry and sends every zero back to zero (below 0, clamped), and 3.0 clamps some."""
    gp = (0.55 + 0.9 * fw.uniform01("grid.gp", L, 91)).astype(np.float32)
    gp[np.flatnonzero(voiced)[:2]] = (0.55, 1.45)  # (the extremes are there whatever the draw)
    ge = (0.5 + fw.uniform01("grid.ge", L, 92)).astype(np.float32)
    return gp, ge


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_grid_equals_forward_per_variant_and_reports_the_realised_variance(models_dir, monkeypatch, precision):
    tts = _tts(models_dir, monkeypatch, precision)
    feats = phones_to_features(PHONES_20)
    L = feats.shape[0]
    assert L == 20
    voiced = feats[:, ref.F_VOICED] == 1
    gp, ge = _grid_gold(L, voiced)
    D, P, E = (1.0, 1.2), (1.5, 3.0), (1.0, 0.8)
    # the CPU side of the choice: at 1.5 the non-zero set is unchanged and nothing non-zero clamps (ratio scale^2), at 3.0 entries clamp
    p0, _, _ = ref.control_one(feats, gp, ge, np.zeros(L, dtype=np.int64), None)
    v0 = ref.stats_one(p0, np.zeros(L), np.zeros(L))
    for s, exact in ((1.5, True), (3.0, False)):
        ps = ref.scale_variance(p0, s)
        vs = ref.stats_one(ps, np.zeros(L), np.zeros(L))
        if exact:
            assert np.array_equal(ps != 0, p0 != 0) and vs[2] / v0[2] == pytest.approx(s * s, rel=1e-12)
        else:
            assert vs[0] < v0[0] and vs[2] / v0[2] < s * s
    variants = prosody.grid(D, P, E)
    zs = [torch.from_numpy(syn.postflow_noise(60 + k, 512)) for k in range(len(variants))]
    gpt, get = torch.from_numpy(gp), torch.from_numpy(ge)
    res = tts.synthesize_grid(PHONES_20, D, P, E, pitch=gpt, energy=get, z_noise=zs)
    assert [r["scales"] for r in res] == variants and len(res) == 8
    for k, r in enumerate(res):
        d, p, e, pause = r["scales"]
        one = tts(PHONES_20, input_is_phones=True, pitch=gpt, energy=get, z_noise=zs[k], duration_scaling_factor=d, pitch_variance_scale=p,
                  energy_variance_scale=e, pause_duration_scaling_factor=pause)
        assert r["wave"].shape == one.shape and r["frames"] * 384 == one.numel()
        assert r["stats_after"][6] in (r["frames"], r["frames"] + 1)  # (the flow's squeeze drops an odd last frame)
        if precision == "bf16":
            assert torch.equal(r["wave"], one), k
        else:
            print(f"fp32, variant {k}: wav max {float((r['wave'] - one).abs().max()):.3e}")
            assert float((r["wave"] - one).abs().max()) < 5e-4, k
        ratio = float(r["stats_after"][2]) / float(r["stats_before"][2])
        print(f"variant {k} {r['scales']}: realised pitch variance ratio {ratio:.6f} (requested {p * p})")
        assert r["stats_before"][0] == int(voiced.sum())
        if p == 1.5:
            assert r["stats_after"][0] == r["stats_before"][0]
            assert abs(ratio - p * p) <= 1e-5 * p * p, k
        else:
            assert r["stats_after"][0] < r["stats_before"][0] and ratio < p * p, k
