"""Per-phoneme prosody curves on a real MI355X (include/toucan_prosody_curves.h):
 (1) tts_prosody_control_c with constant tables against the scalar tts_prosody_control on every utterance alone, and with neutral
     tables against tts_prosody_control_v - bit for bit, NaNs included;
 (2) mixed tables against the float64 restatement (tests/prosody_curves_ref.py), neutral rows untouched, batch == alone;
 (3) tts_prosody_stats over span ranges against the restatement, and a span in a batch == the span alone;
 (4) the stage entry (native.NativePipeline.forward with prosody_curves) against every utterance alone with its scalars, against the
     Python sequencer, and the Python sequencer under use_graphs: one captured stage-A graph for two tables;
 (5) one call with curves against the two-pass route it replaces: predict, read back, re-synthesise with gold prosody;
 (6) the interface: forward == synthesize_batch, synthesize_grid(curves=...) == forward per variant, span statistics, distributed.
fp32 tolerances of a batch against an utterance alone (mel max-abs 5e-4 / mean-abs 1e-4, waveform max-abs 5e-4): the fp32 figures of
tests/test_gpu_native_pipeline.py; the 16-bit configurations are bit-identical whatever the batch."""
import numpy as np
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import capi, engine, fixture_weights as fw, native, prosody, synthetic as syn
from ims_toucan_prosody_variance_amd.phonemes import phones_to_features
from ims_toucan_prosody_variance_amd.prosody import Span
from ims_toucan_prosody_variance_amd.ragged import Ragged
from tests import prosody_curves_ref as cref, prosody_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_LANG = 20
EPS32 = 2.0 ** -23


def _bits(t):
    return t.view(torch.int32)


# ---- (1), (2), (3): the kernels --------------------------------------------------------------------------------------------------------
LENGTHS = [1, 7, 257, 1000]  # one row; less than a sweep; a sweep of 256 and a tail of one; several sweeps and a tail
UNVOICED = 2                 # this utterance has no voiced phoneme: the mean of nothing, NaN wherever its pitch is scaled
CONSTS = [(1.0, 1.3, 1.0), (0.9, 1.0, 0.8), (1.2, 1.5, 1.0), (1.5, 0.6, 2.0)]  # constant (duration, pitch, energy) per utterance, exact 1.0 among them
SCALES = [(1.0, 1.3, 1.0, 0.7), (0.9, 1.0, 0.8, 1.0), (1.2, 1.5, 1.0, 1.3), (1.0, 1.0, 1.0, 1.0)]  # (duration, pitch, energy, pause)
UP = dict(duration=1.3, pitch=1.6, energy=1.4, pitch_offset=0.2, energy_offset=-5.0)    # above 1; the energy offset clamps every row it meets
DOWN = dict(duration=0.7, pitch=0.5, energy=0.6, pitch_offset=-0.15, energy_offset=0.1)  # below 1


def _two_spans(n):
    """Two disjoint spans of an utterance of n rows (the second is empty when n == 1); at n = 1000 both cross a sweep of 256."""
    a0 = n // 8
    b0 = min(n, n // 2 + 1)
    return (a0, a0 + max(1, n // 4)), (b0, min(n, b0 + max(1, n // 3)))


def _mixed():
    lists = [[Span(*_two_spans(n)[0], **UP), Span(*_two_spans(n)[1], **DOWN)] for n in LENGTHS]
    return prosody.resolve_curves(LENGTHS, lists)


@pytest.fixture(scope="module")
def kernel_batch():
    rng = np.random.default_rng(29)
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


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_constant_and_neutral_tables_equal_the_scalar_and_the_per_utterance_kernel(kernel_batch):
    ops = engine.Ops(DEV)
    rag = Ragged(LENGTHS, DEV)
    # constant tables, scales NULL: tts_prosody_control on each utterance alone with those scalars (1 * c == c)
    text, p, e, d = _dev(kernel_batch)
    ops.prosody_control_c(text, p, e, d, rag, None, _t(cref.constant(LENGTHS, CONSTS)))
    for u, (b, n) in enumerate(zip(rag.begins, rag.lengths)):
        tu, pu, eu, du = _dev(kernel_batch, slice(b, b + n))
        ops.prosody_control(tu, pu, eu, du, Ragged([n], DEV), *CONSTS[u], 1.0)
        assert torch.equal(d[b:b + n], du), u
        assert torch.equal(_bits(p[b:b + n]), _bits(pu)), u
        assert torch.equal(_bits(e[b:b + n]), _bits(eu)), u
        if u == UNVOICED:
            assert torch.isnan(pu).all()  # (the NaN of an utterance without a non-zero entry is part of the agreement)
        else:
            assert torch.isfinite(pu).all() and torch.isfinite(eu).all()
    # all-neutral tables with per-utterance scales (exact 1.0 among them): tts_prosody_control_v
    scales = torch.tensor(SCALES, dtype=torch.float32, device=DEV)
    text, p, e, d = _dev(kernel_batch)
    ops.prosody_control_c(text, p, e, d, rag, scales, _t(cref.neutral(sum(LENGTHS))))
    t1, p1, e1, d1 = _dev(kernel_batch)
    ops.prosody_control_v(t1, p1, e1, d1, rag, scales)
    assert torch.equal(d, d1) and torch.equal(_bits(p), _bits(p1)) and torch.equal(_bits(e), _bits(e1))
    assert torch.isnan(p1[rag.begins[UNVOICED]:rag.begins[UNVOICED] + LENGTHS[UNVOICED]]).all()
    # neutral table, no scales: the overrides alone
    text, p, e, d = _dev(kernel_batch)
    ops.prosody_control_c(text, p, e, d, rag, None, _t(cref.neutral(sum(LENGTHS))))
    t1, p1, e1, d1 = _dev(kernel_batch)
    ops.prosody_control_v(t1, p1, e1, d1, rag, None)
    assert torch.equal(d, d1) and torch.equal(_bits(p), _bits(p1)) and torch.equal(_bits(e), _bits(e1))


@pytest.mark.parametrize("with_scales", [False, True])
def test_mixed_tables_match_the_restatement_and_leave_neutral_rows_alone(kernel_batch, with_scales):
    """Durations: equal (the restatement does the same fp32 products and rint).  Pitch / energy: within (n + 6) eps (1 + |s|) max|v|,
    the bound tests/test_prosody_scales_cpu.py derives for (v - avg) s + avg, with |s| the largest effective scale of the utterance,
    plus one fp32 rounding of the offset add: half an ulp of |v' + o| <= (1 + 2 |s|) max|v| + max|o|, i.e. eps / 2 of that."""
    ops = engine.Ops(DEV)
    rag = Ragged(LENGTHS, DEV)
    table, ranges, _ = _mixed()
    scales = np.float32(SCALES) if with_scales else None
    text, p, e, d = _dev(kernel_batch)
    ops.prosody_control_c(text, p, e, d, rag, _t(scales), _t(table))
    kb = kernel_batch
    gp, ge, gd = cref.control(kb["text"], kb["pitch"], kb["energy"], kb["dur"], LENGTHS, scales, table)
    assert np.array_equal(d.cpu().numpy(), gd)
    for got, want, raw, col in ((p, gp, kb["pitch"], 1), (e, ge, kb["energy"], 2)):
        got = got.cpu().numpy().astype(np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(want)), col
        smax = cref.effective_scale(scales, table, LENGTHS, col)
        for u, (b, n) in enumerate(zip(rag.begins, rag.lengths)):
            vmax, omax = float(np.abs(raw[b:b + n]).max()), float(np.abs(table[b:b + n, col + 2]).max())
            tol = (n + 6) * EPS32 * (1 + smax[u]) * vmax + 0.5 * EPS32 * ((1 + 2 * smax[u]) * vmax + omax)
            ok = ~np.isnan(want[b:b + n])
            err = float(np.abs(got[b:b + n][ok] - want[b:b + n][ok]).max()) if ok.any() else 0.0
            print(f"scales {with_scales}, column {col}, utterance {u}: max err {err:.3e}, bound {tol:.3e}, NaN rows {int((~ok).sum())}")
            assert err <= tol, (u, col)
    b = rag.begins[UNVOICED]
    assert np.isnan(gp[b:b + LENGTHS[UNVOICED]]).any() and (ge[table[:, 4] == -5.0] == 0).all()  # the NaN mean and the clamping offset are in the case
    # every utterance of the batch == the utterance alone, bit for bit
    for u, (b, n) in enumerate(zip(rag.begins, rag.lengths)):
        tu, pu, eu, du = _dev(kernel_batch, slice(b, b + n))
        ops.prosody_control_c(tu, pu, eu, du, Ragged([n], DEV), _t(None if scales is None else scales[u:u + 1]), _t(table[b:b + n]))
        assert torch.equal(d[b:b + n], du) and torch.equal(_bits(p[b:b + n]), _bits(pu)) and torch.equal(_bits(e[b:b + n]), _bits(eu)), u
    if not with_scales:  # rows that are neutral under S = 1 keep the bits the overrides left, whatever the spans beside them do
        t0, p0, e0, d0 = _dev(kernel_batch)
        ops.prosody_control_v(t0, p0, e0, d0, rag, None)
        same = torch.from_numpy((table == cref.NEUTRAL).all(axis=1)).to(DEV)
        assert 0 < int(same.sum()) < same.numel()
        assert torch.equal(d[same], d0[same]) and torch.equal(_bits(p[same]), _bits(p0[same])) and torch.equal(_bits(e[same]), _bits(e0[same]))
        assert not torch.equal(d[~same], d0[~same]) and not torch.equal(_bits(e[~same]), _bits(e0[~same]))


def test_span_statistics_match_the_restatement_and_do_not_depend_on_the_batch(kernel_batch):
    ops = engine.Ops(DEV)
    rag = Ragged(LENGTHS, DEV)
    table, ranges, _ = _mixed()
    assert ranges.shape == (8, 2) and ranges[1, 0] == ranges[1, 1]  # (the one-row utterance's second span is empty)
    text, p, e, d = _dev(kernel_batch)
    dev_ranges = _t(ranges.T)
    for step in ("overrides", "curves"):
        if step == "overrides":
            ops.prosody_control_v(text, p, e, d, rag, None)
        else:
            ops.prosody_control_c(text, p, e, d, rag, None, _t(table))
        got = ops.prosody_span_stats(p, e, d, dev_ranges, torch.full((8, capi.PROSODY_STATS), -7.0, device=DEV))
        ph, eh, dh = p.cpu().numpy(), e.cpu().numpy(), d.cpu().numpy()
        want = np.stack([ref.stats_one(ph[a:b], eh[a:b], dh[a:b]) for a, b in ranges])
        print("span stats after the", step, "\n", got.cpu().numpy(), "\n", want)
        ref.assert_stats_match(got.cpu().numpy(), want)  # counts, frames and rows exact; means and variances to 1e-6 relative
        assert np.array_equal(want[1], np.zeros(8))
        for k, (a, b) in enumerate(ranges):
            if b > a:
                alone = ops.prosody_stats(p[a:b].clone(), e[a:b].clone(), d[a:b].clone(), Ragged([b - a], DEV),
                                          torch.full((1, capi.PROSODY_STATS), -7.0, device=DEV))
                assert torch.equal(_bits(alone[0]), _bits(got[k])), k
    assert np.isnan(want[2 * UNVOICED, 1])  # the scaled span of the unvoiced utterance carries the NaN mean


# ---- (4), (5): the stage entry and the Python sequencer -----------------------------------------------------------------------------
US, LS = [300, 301, 302], [7, 20, 20]
STAGE_CONSTS = [(1.2, 1.3, 1.0), (0.9, 1.0, 0.8), (1.0, 1.5, 1.25)]
# Spans on rows that are voiced phonemes in synthetic.utterance_features (rows 1-3; 1-3 and 5-7; 1-7 and 13-15), factors >= 1:
# the route of test (5) needs zeros to stay zeros, and the fixture weights predict NEGATIVE means, under which a zero inside a span
# scaled above 1 would not (it becomes avg (1 - es) > 0) - so its spans hold no zero.  The tests assert that premise.
EDIT_CURVES = [[Span(1, 4, duration=1.5, pitch=1.4, energy=1.2, pitch_offset=0.1)],
               [Span(1, 4, pitch=1.3, energy_offset=0.2), Span(5, 8, duration=1.25, energy=1.5)],
               [Span(1, 8, duration=1.1, pitch=2.0, pitch_offset=-0.05), Span(13, 16, duration=2.0, energy=1.1, energy_offset=-0.1), Span(3, 6, pitch=1.2)]]
OTHER_CURVES = [[Span(0, 7, duration=0.8, pitch=0.5, energy=0.7)],
                [Span(9, 16, duration=1.4, pitch=1.6, energy=1.3), Span(1, 8, energy=0.5, pitch_offset=0.3)],
                [Span(17, 18, duration=3.0), Span(1, 8, pitch=0.9), Span(9, 16, energy_offset=0.05)]]  # the same span counts: the same shape


def _stage_inputs():
    feats = [torch.from_numpy(syn.utterance_features(u, L)) for u, L in zip(US, LS)]
    embs = torch.from_numpy(np.stack([syn.utterance_embedding(u) for u in US]))
    zs = [torch.from_numpy(syn.postflow_noise(u, 512)) for u in US]
    return feats, embs, [syn.LANG_EN] * 3, zs


@pytest.fixture(scope="module", params=["bf16", "f32"])
def stage(request):
    precision = request.param
    ac_sd, voc_sd = fw.acoustic_state_dict(), fw.bigvgan_state_dict()
    pipe = native.NativePipeline(ac_sd, voc_sd, "bigvgan", DEV, precision=precision)
    return dict(precision=precision, pipe=pipe, ac_sd=ac_sd, voc_sd=voc_sd)


def _same_prosody(a, b, u, ua=None):
    ua = u if ua is None else ua
    assert torch.equal(a["durations"][ua], b["durations"][u]), u
    assert torch.equal(_bits(a["pitch"][ua]), _bits(b["pitch"][u])), u
    assert torch.equal(_bits(a["energy"][ua]), _bits(b["energy"][u])), u


def test_stage_constant_tables_equal_every_utterance_alone_with_its_scalars(stage):
    pipe = stage["pipe"]
    feats, embs, langs, zs = _stage_inputs()
    consts = [np.tile(np.float32(list(c) + [0, 0]), (L, 1)) for c, L in zip(STAGE_CONSTS, LS)]
    out = pipe.forward(feats, embs, langs, z_noise=zs, prosody_curves=consts)
    wav = out["wav"]
    assert out["prosody_stats"][0].shape == (3, 8) and [tuple(b.shape) for b, _ in out["prosody_span_stats"]] == [(0, 8)] * 3
    for u in range(3):
        d, p, e = STAGE_CONSTS[u]
        one = pipe.forward([feats[u]], embs[u:u + 1], [langs[u]], z_noise=[zs[u]], duration_scaling_factor=d, pitch_variance_scale=p,
                           energy_variance_scale=e)
        assert "prosody_stats" not in one and "prosody_span_stats" not in one  # (the scalar entry)
        _same_prosody(one, out, u, 0)
        b, n = out["wav_spans"][u]
        b1, n1 = one["wav_spans"][0]
        assert n == n1 and one["mel"][0].shape == out["mel"][u].shape
        if stage["precision"] == "bf16":  # the 16-bit contract: bit for bit whatever the batch
            assert torch.equal(one["mel"][0], out["mel"][u]), u
            assert torch.equal(one["wav"][b1:b1 + n1], wav[b:b + n]), u
        else:
            err = (one["mel"][0] - out["mel"][u]).abs()
            werr = float((one["wav"][b1:b1 + n1] - wav[b:b + n]).abs().max())
            print(f"fp32, utterance {u}: mel max {float(err.max()):.3e} mean {float(err.mean()):.3e}, wav max {werr:.3e}")
            assert float(err.max()) < 5e-4 and float(err.mean()) < 1e-4, u
            assert werr < 5e-4, u
    # scalars of the call multiply the table: the constant table under a scalar pitch scale == the product given as the table
    scaled = pipe.forward(feats, embs, langs, z_noise=zs, prosody_curves=consts, pitch_variance_scale=2.0, vocode=False)
    twice = [c * np.float32([1, 2, 1, 1, 1]) for c in consts]
    direct = pipe.forward(feats, embs, langs, z_noise=zs, prosody_curves=twice, vocode=False)
    for u in range(3):
        _same_prosody(scaled, direct, u)


def test_python_sequencer_and_its_graphs_equal_the_stage_entry(stage):
    pipe, precision = stage["pipe"], stage["precision"]
    feats, embs, langs, zs = _stage_inputs()
    outs = [pipe.forward(feats, embs, langs, z_noise=zs, prosody_curves=c, vocode=False) for c in (EDIT_CURVES, OTHER_CURVES)]
    assert not torch.equal(outs[0]["durations_packed"], outs[1]["durations_packed"])

    def same(py, out):
        for u in range(3):
            _same_prosody(py, out, u)
            assert torch.equal(py["mel"][u], out["mel"][u]), u
        for a, b in list(zip(py["prosody_stats"], out["prosody_stats"])) + [ab for pu, ou in zip(py["prosody_span_stats"], out["prosody_span_stats"])
                                                                             for ab in zip(pu, ou)]:
            assert a.dtype == b.dtype == np.float32 and a.shape == b.shape
            assert np.array_equal(a.view(np.int32), b.view(np.int32))

    ac = engine.AcousticEngine(stage["ac_sd"], DEV, precision=precision)
    for c, out in zip((EDIT_CURVES, OTHER_CURVES), outs):
        same(ac.forward(feats, embs, langs, z_noise=zs, prosody_curves=c), out)
    # the statistics against the restatement: "before" from a pass without curves, "after" from the batch's own result
    out = outs[0]
    plain = pipe.forward(feats, embs, langs, run_postflow=False, vocode=False)
    cat = lambda o, k: torch.cat(o[k]).cpu().numpy()
    before, after = out["prosody_stats"]
    ref.assert_stats_match(before, ref.stats(cat(plain, "pitch"), cat(plain, "energy"), cat(plain, "durations"), LS))
    ref.assert_stats_match(after, ref.stats(cat(out, "pitch"), cat(out, "energy"), cat(out, "durations"), LS))
    assert [tuple(b.shape) for b, _ in out["prosody_span_stats"]] == [(1, 8), (2, 8), (3, 8)]
    for u, spans in enumerate(EDIT_CURVES):
        sb, sa = out["prosody_span_stats"][u]
        for k, s in enumerate(spans):
            sl = slice(s.start, s.stop)
            for o, blocks in ((plain, sb), (out, sa)):
                want = ref.stats_one(o["pitch"][u][sl].cpu().numpy(), o["energy"][u][sl].cpu().numpy(), o["durations"][u][sl].cpu().numpy())
                ref.assert_stats_match(blocks[k:k + 1], want[None])
            assert sa[k, 6] == int(out["durations"][u][sl].sum()) and sa[k, 7] == s.stop - s.start  # column 6: the frames the span occupies
    # use_graphs: two tables of one shape replay ONE captured stage-A graph, and both equal the results without graphs
    acg = engine.AcousticEngine(stage["ac_sd"], DEV, precision=precision, use_graphs=True)
    for c, out in zip((EDIT_CURVES, OTHER_CURVES, EDIT_CURVES), outs + outs[:1]):
        same(acg.forward(feats, embs, langs, z_noise=zs, prosody_curves=c), out)
    keys_a = [k for k in acg._graphs.entries if k[0] == "A"]
    assert len(keys_a) == 1 and "curves" in keys_a[0], keys_a


def test_one_call_with_curves_equals_predict_edit_and_resynthesise(stage):
    """The two-pass route the feature replaces: read the first call's durations / pitch / energy back and give them to a second
    call as gold prosody, without curves.  With factors >= 1 on spans without a zero entry, zeros stay zeros and the second pass's
    overrides find nothing to change, so the two mels and waveforms are the same bits (bf16; fp32 takes the same path here too)."""
    pipe = stage["pipe"]
    feats, embs, langs, zs = _stage_inputs()
    first = pipe.forward(feats, embs, langs, z_noise=zs, prosody_curves=EDIT_CURVES)
    for u, f in enumerate(feats):  # the premise
        assert (first["pitch"][u][f[:, 61].to(DEV) == 0] == 0).all() and (first["energy"][u][f[:, 15].to(DEV) == 0] == 0).all(), u
        assert (first["durations"][u][f[:, 21].to(DEV) == 1] == 0).all(), u
        for s in EDIT_CURVES[u]:
            assert (f[s.start:s.stop, 61] == 1).all() and (f[s.start:s.stop, 15] == 1).all() and min(s.duration, s.pitch, s.energy) >= 1, (u, s)
    second = pipe.forward(feats, embs, langs, z_noise=zs, durations=[d.clone() for d in first["durations"]],
                          pitch=[p.clone() for p in first["pitch"]], energy=[e.clone() for e in first["energy"]])
    assert "prosody_stats" not in second
    for u in range(3):
        _same_prosody(second, first, u)
        assert torch.equal(second["mel"][u], first["mel"][u]), u
        (b, n), (b2, n2) = first["wav_spans"][u], second["wav_spans"][u]
        assert n == n2 and torch.equal(second["wav"][b2:b2 + n2], first["wav"][b:b + n]), u
    plain = pipe.forward(feats, embs, langs, z_noise=zs, vocode=False)
    assert all(int(first["durations"][u].sum()) > int(plain["durations"][u].sum()) for u in range(3))  # (the curves did something)


# ---- (6): the interface ----------------------------------------------------------------------------------------------------------------
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


PHONES_20 = "~wˈʌns əpˈɑːn mˈɪdnaɪt~#"
PHONES_13 = "~həlˈoʊ wˈɜːld~#"


def test_interface_forward_batch_grid_and_span_statistics(models_dir, monkeypatch):
    tts = _tts(models_dir, monkeypatch, "bf16")
    feats = phones_to_features(PHONES_20)
    words = prosody.word_spans(feats)
    assert len(words) == 3 and feats.shape[0] == 20
    z = torch.from_numpy(syn.postflow_noise(70, 512))
    stress = prosody.emphasis(feats, [1], duration=1.3, pitch=1.5, energy=1.2, pitch_offset=0.1)
    # forward == synthesize_batch of the same utterance, alone and beside another one
    one = tts(PHONES_20, input_is_phones=True, z_noise=z, prosody_curves=stress)
    d_one = tts.last_durations[0].clone()
    assert tts.last_prosody_stats[0].shape == (1, 8) and tts.last_prosody_span_stats[0][1].shape == (1, 8)
    plain = tts(PHONES_20, input_is_phones=True, z_noise=z)
    assert tts.last_prosody_stats is None and tts.last_prosody_span_stats is None and one.numel() > plain.numel()
    both = tts.synthesize_batch([PHONES_13, PHONES_20], z_noise=[z, z], prosody_curves=[None, stress])
    assert torch.equal(both[1], one) and torch.equal(tts.last_durations[1], d_one)
    assert [tuple(b.shape) for b, _ in tts.last_prosody_span_stats] == [(0, 8), (1, 8)]
    assert torch.equal(both[0], tts(PHONES_13, input_is_phones=True, z_noise=z))  # (its neighbour's curves leave it alone)
    streamed = torch.cat(list(tts.stream(PHONES_20, input_is_phones=True, z_noise=z, prosody_curves=stress)))
    assert torch.equal(streamed, one)
    # the grid: 2 alternatives x 2 pitch scales, the alternatives slowest; every variant == forward
    curves = [prosody.emphasis(feats, [k], duration=1.3, pitch=1.5, energy=1.2) for k in (0, 2)]
    P = (1.0, 1.3)
    zs = [torch.from_numpy(syn.postflow_noise(80 + k, 512)) for k in range(4)]
    res = tts.synthesize_grid(PHONES_20, pitch_variance_scales=P, curves=curves, z_noise=zs)
    assert [(r["curve"], r["scales"]) for r in res] == [(c, (1.0, p, 1.0, 1.0)) for c in (0, 1) for p in P]
    for k, r in enumerate(res):
        alone = tts(PHONES_20, input_is_phones=True, z_noise=zs[k], pitch_variance_scale=r["scales"][1], prosody_curves=curves[r["curve"]])
        assert torch.equal(r["wave"], alone) and r["frames"] * 384 == alone.numel(), k
        durations = tts.last_durations[0].cpu().numpy()
        a, b = words[(0, 2)[r["curve"]]]
        before, after = r["span_stats"]
        assert before.shape == after.shape == (1, 8) and after[0, 7] == b - a
        in_front, inside = int(durations[:a].sum()), int(durations[a:b].sum())
        print(f"variant {k}: word rows [{a}, {b}) -> frames [{in_front}, {in_front + inside}) of {r['frames']}, {before[0, 6]:.0f} before the curves")
        assert after[0, 6] == inside > before[0, 6] > 0  # column 6: the frames the span occupies, after and before its duration factor
        assert in_front + inside <= r["stats_after"][6] and r["stats_after"][6] in (r["frames"], r["frames"] + 1)
    with pytest.raises(ValueError, match="distributed"):
        tts.synthesize_batch([PHONES_13, PHONES_20], prosody_curves=[None, stress], distributed=True)
