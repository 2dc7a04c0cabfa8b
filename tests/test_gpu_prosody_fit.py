"""Time budgets on a real MI355X (include/toucan_prosody_fit.h):
 (1) tts_prosody_fit against the numpy restatement (tests/prosody_fit_ref.py): value bits, extra, report, both written tables;
 (2) a batch equals every utterance alone, bit for bit;
 (3) exact=False: tts_prosody_control_v with the written scales == the scalar kernel on the utterance alone at the value;
 (4) exact=True: control + apply give every EXACT / REPAIRED segment its target, rows == the scalar kernel's at the value + extra;
 (5) spans with and without an input curve table;
 (6) the stage entry on the seeded fixture weights, bf16 and f32, against the utterance alone and the Python sequencer;
 (7) CLAMPED_* and EMPTY through the interface, and argument errors that enqueue nothing.
Shapes: one row, less than a sweep of 256, a sweep and one, several sweeps (the fixture of tests/prosody_fit_ref.py).  fp32 tolerances of
a batch against an utterance alone (mel max-abs 5e-4 / mean-abs 1e-4): the figures of tests/test_gpu_native_pipeline.py."""
import ctypes

import numpy as np
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import capi, engine, fixture_weights as fw, native, prosody_fit, synthetic as syn
from ims_toucan_prosody_variance_amd.prosody_fit import Fit
from ims_toucan_prosody_variance_amd.ragged import Ragged
from tests import prosody_fit_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONFIGS = [(True, True), (True, False), (False, True), (False, False)]  # (input scales, input curve table)


def _bits(a):
    return a.view(np.int32) if isinstance(a, np.ndarray) else a.view(torch.int32)


@pytest.fixture(scope="module")
def fx():
    f = ref.fixture()
    rng = np.random.default_rng(7)
    R = len(f["dur"])
    f["pitch"] = (0.3 + 0.5 * rng.standard_normal(R)).astype(np.float32)
    f["energy"] = (0.5 + 0.4 * rng.standard_normal(R)).astype(np.float32)
    f["want"] = {cfg: ref.fit(f["text"], f["dur"], f["lengths"], f["segments"], f["scales"] if cfg[0] else None, f["curves"] if cfg[1] else None)
                 for cfg in CONFIGS}  # the restatement, computed once
    return f


def _to(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _fit(ops, text, dur, lengths, segments, scales, curves):
    """tts_prosody_fit on host arrays -> (scales_out, curves_out or None, extra, report) as numpy; the outputs start poisoned."""
    rag = Ragged(lengths, DEV)
    B, R = len(lengths), int(sum(lengths))
    rows, spec = prosody_fit.device_tables(segments)
    need_curves = curves is not None or bool((segments[:, 1] == ref.SPAN).any())
    scales_out = torch.full((B, 4), -7.0, device=DEV)
    curves_out = torch.full((R, 5), -7.0, device=DEV) if need_curves else None
    extra = torch.full((R,), -7, dtype=torch.int32, device=DEV)
    report = torch.full((len(segments), 8), -7.0, device=DEV)
    ops.prosody_fit(_to(text), _to(dur), rag, _to(rows), _to(spec), _to(scales), _to(curves), scales_out, curves_out, extra, report)
    torch.cuda.synchronize()
    return scales_out.cpu().numpy(), None if curves_out is None else curves_out.cpu().numpy(), extra.cpu().numpy(), report.cpu().numpy()


def _tables(fx, cfg):
    return (fx["scales"] if cfg[0] else None), (fx["curves"] if cfg[1] else None)


@pytest.mark.parametrize("cfg", CONFIGS)
def test_fit_equals_the_restatement(fx, cfg):
    ops = engine.Ops(DEV)
    scales, curves = _tables(fx, cfg)
    got = _fit(ops, fx["text"], fx["dur"], fx["lengths"], fx["segments"], scales, curves)
    w_scales, w_curves, w_extra, w_report, solved = fx["want"][cfg]
    print("status", got[3][:, 4].astype(int).tolist(), "iterations", got[3][:, 5].astype(int).tolist())
    assert np.array_equal(_bits(got[3][:, 3]), _bits(w_report[:, 3]))  # the value's bits
    assert np.array_equal(_bits(got[3]), _bits(w_report))
    assert np.array_equal(got[2], w_extra)
    assert np.array_equal(_bits(got[0]), _bits(w_scales)) and np.array_equal(_bits(got[1]), _bits(w_curves))
    # utterances and rows without a segment keep their input bits (or the neutral values)
    begins = np.concatenate([[0], np.cumsum(fx["lengths"])])
    u = ref.UNFITTED
    assert np.array_equal(got[0][u], scales[u] if scales is not None else np.ones(4, dtype=np.float32))
    neutral = np.tile(np.float32([1, 1, 1, 0, 0]), (len(fx["dur"]), 1))
    assert np.array_equal(_bits(got[1][begins[u]:begins[u + 1]]), _bits((curves if curves is not None else neutral)[begins[u]:begins[u + 1]]))
    assert not got[2][begins[u]:begins[u + 1]].any()


@pytest.mark.parametrize("cfg", [(True, True), (False, False)])
def test_batch_equals_every_utterance_alone(fx, cfg):
    ops = engine.Ops(DEV)
    scales, curves = _tables(fx, cfg)
    s_all, c_all, e_all, r_all = _fit(ops, fx["text"], fx["dur"], fx["lengths"], fx["segments"], scales, curves)
    begins = np.concatenate([[0], np.cumsum(fx["lengths"])])
    for u, n in enumerate(fx["lengths"]):
        which = np.flatnonzero(fx["segments"][:, 0] == u)
        if len(which) == 0:
            continue
        b = int(begins[u])
        seg = fx["segments"][which].copy()
        seg[:, 0] = 0
        seg[:, 2:4] -= b
        sl = slice(b, b + n)
        s1, c1, e1, r1 = _fit(ops, fx["text"][sl], fx["dur"][sl], [n], seg, None if scales is None else scales[u:u + 1],
                              None if curves is None else curves[sl])
        assert np.array_equal(_bits(r1), _bits(r_all[which])), u
        assert np.array_equal(_bits(s1[0]), _bits(s_all[u])) and np.array_equal(e1, e_all[sl]), u
        if c1 is not None:
            assert np.array_equal(_bits(c1), _bits(c_all[sl])), u


def _control(ops, fx, lengths, sl, scales=None, curves=None, scalars=None):
    """The control kernel on rows sl of the fixture -> (durations, pitch, energy) on the device."""
    rag = Ragged(lengths, DEV)
    text, p, e, d = (_to(fx[k][sl].copy()) for k in ("text", "pitch", "energy", "dur"))
    if scalars is not None:
        ops.prosody_control(text, p, e, d, rag, *[float(v) for v in scalars])
    elif curves is not None:
        ops.prosody_control_c(text, p, e, d, rag, _to(scales), _to(curves))
    else:
        ops.prosody_control_v(text, p, e, d, rag, _to(scales))
    return d, p, e


@pytest.mark.parametrize("exact", [0, 1])
def test_written_scales_under_the_control_kernel(fx, exact):
    """(3) and (4): whole-utterance segments without a curve table, all NEAREST-able (exact 0) or all repaired (exact 1)."""
    ops = engine.Ops(DEV)
    seg = fx["segments"][fx["segments"][:, 1] != ref.SPAN].copy()
    seg[:, 7] = exact
    scales = fx["scales"]
    s_out, c_out, extra, report = _fit(ops, fx["text"], fx["dur"], fx["lengths"], seg, scales, None)
    assert c_out is None
    status = report[:, 4].astype(int)
    if exact:
        assert ref.NEAREST not in status and ref.REPAIRED in status
    else:
        assert ref.REPAIRED not in status and ref.NEAREST in status and not extra.any()
    d, p, e = _control(ops, fx, fx["lengths"], slice(None), scales=s_out)
    ops.prosody_fit_apply(d, _to(extra))
    begins = np.concatenate([[0], np.cumsum(fx["lengths"])])
    for s, g in enumerate(seg):
        u, n = int(g[0]), fx["lengths"][int(g[0])]
        sl = slice(int(begins[u]), int(begins[u]) + n)
        du, pu, eu = _control(ops, fx, [n], sl, scalars=s_out[u])
        assert torch.equal(d[sl], du + _to(extra[sl])), u
        assert torch.equal(_bits(p[sl]), _bits(pu)) and torch.equal(_bits(e[sl]), _bits(eu)), u
        assert report[s, 3] == s_out[u, 0 if g[1] == ref.UTT_DURATION else 3] or status[s] == ref.EMPTY
        if status[s] in (ref.EXACT, ref.REPAIRED):
            assert int(d[sl].sum()) == int(g[4]) == int(report[s, 1]), u
        assert int(d[sl].sum()) == int(report[s, 1]), u


@pytest.mark.parametrize("with_table", [True, False])
def test_spans(fx, with_table):
    """(5) kernel level: a span takes its target, rows outside spans keep the bits of the call without a fit."""
    ops = engine.Ops(DEV)
    seg = fx["segments"][fx["segments"][:, 1] == ref.SPAN]
    scales, curves = fx["scales"], (fx["curves"] if with_table else None)
    s_out, c_out, extra, report = _fit(ops, fx["text"], fx["dur"], fx["lengths"], seg, scales, curves)
    assert np.array_equal(_bits(s_out), _bits(scales))  # spans write no scale
    d0, p0, e0 = _control(ops, fx, fx["lengths"], slice(None), scales=scales, curves=curves)
    d1, p1, e1 = _control(ops, fx, fx["lengths"], slice(None), scales=scales, curves=c_out)
    ops.prosody_fit_apply(d1, _to(extra))
    inside = np.zeros(len(fx["dur"]), dtype=bool)
    hit = 0
    for s, g in enumerate(seg):
        b, e = int(g[2]), int(g[3])
        inside[b:e] = True
        assert int(d1[b:e].sum()) == int(report[s, 1])
        if int(report[s, 4]) in (ref.EXACT, ref.REPAIRED):
            assert int(d1[b:e].sum()) == int(g[4])
            hit += 1
    assert hit >= 3
    outside = _to(~inside)
    assert torch.equal(d1[outside], d0[outside])
    assert torch.equal(_bits(p1), _bits(p0)) and torch.equal(_bits(e1), _bits(e0))  # (column 0 alone was rewritten)


# ---- (6): the stage entry and the Python sequencer -----------------------------------------------------------------------------------
US, LS = [310, 311, 312], [20, 33, 9]


def _stage_inputs():
    feats = [torch.from_numpy(syn.utterance_features(u, L)) for u, L in zip(US, LS)]
    embs = torch.from_numpy(np.stack([syn.utterance_embedding(u) for u in US]))
    zs = [torch.from_numpy(syn.postflow_noise(u, 2048)) for u in US]
    return feats, embs, [syn.LANG_EN] * 3, zs


@pytest.fixture(scope="module", params=["bf16", "f32"])
def stage(request):
    precision = request.param
    ac_sd = fw.acoustic_state_dict()
    pipe = native.NativePipeline(ac_sd, None, None, DEV, precision=precision)
    feats, embs, langs, zs = _stage_inputs()
    plain = pipe.forward(feats, embs, langs, z_noise=zs, vocode=False)
    base = [int(d.sum()) for d in plain["durations"]]
    sil = int(plain["durations"][1][feats[1][:, ref.F_SILENCE] == 1].sum())
    print(f"{precision}: frames without a fit {base}, frames of utterance 1's pauses {sil}")
    assert sil > 0 and min(base) > 0  # (the fixture weights predict pauses that a pause fit can stretch)
    targets = [int(round(1.37 * base[0])), base[1] + 2 * sil + 1, None]
    fits = [Fit(target_frames=targets[0]), Fit(target_seconds=targets[1] / 62.5, knob="pause"), None]
    out = pipe.forward(feats, embs, langs, z_noise=zs, vocode=False, prosody_fit=fits)
    return dict(precision=precision, pipe=pipe, ac_sd=ac_sd, plain=plain, out=out, targets=targets, fits=fits)


def _close(a, b, precision, what):
    if precision == "bf16":
        assert torch.equal(a, b), what
    else:
        err = (a - b).abs()
        print(f"fp32, {what}: mel max {float(err.max()):.3e} mean {float(err.mean()):.3e}")
        assert float(err.max()) < 5e-4 and float(err.mean()) < 1e-4, what


def test_stage_fits_hit_their_targets(stage):
    out, plain, targets = stage["out"], stage["plain"], stage["targets"]
    fit = out["prosody_fit"]
    print("report", [r.tolist() for r in fit["report"]], "scales", fit["scales"].tolist())
    assert [r.shape for r in fit["report"]] == [(1, 8), (1, 8), (0, 8)] and fit["scales"].shape == (3, 4) and [len(e) for e in fit["extra"]] == LS
    for u in (0, 1):
        r = fit["report"][u][0]
        assert int(r[4]) in (ref.EXACT, ref.REPAIRED) and r[0] == r[1] == targets[u], u
        assert int(out["durations"][u].sum()) == targets[u] == out["rag_frame"].lengths[u], u
        assert r[7] == int(plain["durations"][u].sum()), u
        assert fit["scales"][u, 0 if u == 0 else 3] == r[3] and fit["scales"][u, 3 if u == 0 else 0] == 1.0, u
    assert np.array_equal(fit["scales"][2], np.ones(4, dtype=np.float32)) and not fit["extra"][2].any()
    before, after = out["prosody_stats"]
    assert np.array_equal(after[:2, 6], np.float32(targets[:2])) and after[2, 6] == int(plain["durations"][2].sum())
    assert np.array_equal(before[:, 6], [int(d.sum()) for d in plain["durations"]])
    # the utterance without a Fit is the utterance of the same batch without prosody_fit
    assert torch.equal(out["durations"][2], plain["durations"][2])
    assert torch.equal(_bits(out["pitch"][2]), _bits(plain["pitch"][2])) and torch.equal(_bits(out["energy"][2]), _bits(plain["energy"][2]))
    _close(out["mel"][2], plain["mel"][2], stage["precision"], "the utterance without a Fit")
    assert "prosody_fit" not in plain and "prosody_stats" not in plain


def test_stage_fitted_utterance_equals_its_durations_given_alone(stage):
    pipe, out = stage["pipe"], stage["out"]
    feats, embs, langs, zs = _stage_inputs()
    for u in (0, 1):
        one = pipe.forward([feats[u]], embs[u:u + 1], [langs[u]], z_noise=[zs[u]], vocode=False, durations=[out["durations"][u].cpu()])
        assert torch.equal(one["durations"][0], out["durations"][u]), u
        assert torch.equal(_bits(one["pitch"][0]), _bits(out["pitch"][u])) and torch.equal(_bits(one["energy"][0]), _bits(out["energy"][u])), u
        _close(one["mel"][0], out["mel"][u], stage["precision"], f"fitted utterance {u}")


def test_stage_span_fit_and_the_python_sequencer(stage):
    pipe, precision = stage["pipe"], stage["precision"]
    feats, embs, langs, zs = _stage_inputs()
    ac = engine.AcousticEngine(stage["ac_sd"], DEV, precision=precision)
    py = ac.forward(feats, embs, langs, z_noise=zs, prosody_fit=stage["fits"])
    out = stage["out"]
    for u in range(3):
        assert torch.equal(py["durations"][u], out["durations"][u]) and torch.equal(py["mel"][u], out["mel"][u]), u
        assert np.array_equal(_bits(py["prosody_fit"]["report"][u]), _bits(out["prosody_fit"]["report"][u])), u
        assert np.array_equal(py["prosody_fit"]["extra"][u], out["prosody_fit"]["extra"][u]), u
    assert np.array_equal(_bits(py["prosody_fit"]["scales"]), _bits(out["prosody_fit"]["scales"]))
    for a, b in zip(py["prosody_stats"], out["prosody_stats"]):
        assert np.array_equal(_bits(a), _bits(b))
    if precision == "bf16":  # the captured form of the Python sequencer: the capture, then a replay with other targets
        acg = engine.AcousticEngine(stage["ac_sd"], DEV, precision=precision, use_graphs=True)
        g = acg.forward(feats, embs, langs, z_noise=zs, prosody_fit=[Fit(target_frames=stage["targets"][0] + 9), Fit(target_frames=stage["targets"][1] - 1, knob="pause"), None])
        assert [int(d.sum()) for d in g["durations"][:2]] == [stage["targets"][0] + 9, stage["targets"][1] - 1]
        g = acg.forward(feats, embs, langs, z_noise=zs, prosody_fit=stage["fits"])
        for u in range(3):
            assert torch.equal(g["durations"][u], out["durations"][u]) and torch.equal(g["mel"][u], out["mel"][u]), u
            assert np.array_equal(_bits(g["prosody_fit"]["report"][u]), _bits(out["prosody_fit"]["report"][u])), u
    # spans, with an input curve table on utterance 1 and per-utterance scales: both sequencers, and the _c entry given the written table
    plain = stage["plain"]
    rng = np.random.default_rng(3)
    table = np.tile(np.float32([1, 1, 1, 0, 0]), (LS[1], 1))
    table[:, 0] = (0.7 + 0.6 * rng.random(LS[1])).astype(np.float32)
    curves = [None, table, None]
    kw = dict(duration_scaling_factor=[1.1, 0.9, 1.0], pitch_variance_scale=1.2)
    spans = [(0, 1, 8), (1, 2, 17), (1, 20, 31)]
    given = pipe.forward(feats, embs, langs, z_noise=zs, vocode=False, prosody_curves=curves, **kw)
    t = [int(round(f * int(given["durations"][u][a:b].sum()))) for f, (u, a, b) in zip((1.4, 0.7, 1.25), spans)]
    fits = [[Fit(t[0], start=1, stop=8)], [Fit(t[1], start=2, stop=17), Fit(t[2], start=20, stop=31)], None]
    got = pipe.forward(feats, embs, langs, z_noise=zs, vocode=False, prosody_curves=curves, prosody_fit=fits, **kw)
    py = ac.forward(feats, embs, langs, z_noise=zs, prosody_curves=curves, prosody_fit=fits, **kw)
    print("span targets", t, "report", [r.tolist() for r in got["prosody_fit"]["report"]])
    values = {}
    for k, (u, a, b) in enumerate(spans):
        r = got["prosody_fit"]["report"][u][k - (1 if u else 0)]
        assert int(r[4]) in (ref.EXACT, ref.REPAIRED) and int(got["durations"][u][a:b].sum()) == t[k] == r[0], k
        values[(u, a, b)] = np.float32(r[3])
    for u in range(3):
        inside = np.zeros(LS[u], dtype=bool)
        for (v, a, b) in spans:
            if v == u:
                inside[a:b] = True
        keep = torch.from_numpy(~inside).to(DEV)
        assert torch.equal(got["durations"][u][keep], given["durations"][u][keep]), u  # rows outside spans: the call without a fit
        assert torch.equal(_bits(got["pitch"][u]), _bits(given["pitch"][u])) and torch.equal(_bits(got["energy"][u]), _bits(given["energy"][u])), u
        assert torch.equal(py["durations"][u], got["durations"][u]) and torch.equal(py["mel"][u], got["mel"][u]), u
        assert np.array_equal(_bits(py["prosody_fit"]["report"][u]), _bits(got["prosody_fit"]["report"][u])), u
    _close(got["mel"][2], given["mel"][2], precision, "span batch, the utterance without a Fit")
    # tts_control_and_regulate_c given the written curve table reproduces the durations before the extra frames
    written = [np.tile(np.float32([1, 1, 1, 0, 0]), (L, 1)) for L in LS]
    written[1] = table.copy()
    for (u, a, b), v in values.items():
        written[u][a:b, 0] = written[u][a:b, 0] * v
    again = pipe.forward(feats, embs, langs, z_noise=zs, vocode=False, prosody_curves=written, **kw)
    for u in range(3):
        extra = torch.from_numpy(got["prosody_fit"]["extra"][u]).to(DEV)
        assert torch.equal(again["durations"][u] + extra, got["durations"][u]), u
    assert np.array_equal(_bits(got["prosody_fit"]["scales"]), _bits(np.float32([[1.1, 1.2, 1, 1], [0.9, 1.2, 1, 1], [1.0, 1.2, 1, 1]])))
    assert plain is not None


# ---- (7): the interface ------------------------------------------------------------------------------------------------------------------
PHONES_20 = "~wˈʌns əpˈɑːn mˈɪdnaɪt~#"
PHONES_13 = "~həlˈoʊ wˈɜːld~#"


@pytest.fixture(scope="module")
def models_dir(tmp_path_factory):
    from ims_toucan_prosody_variance_amd import interface
    d = tmp_path_factory.mktemp("Models")
    interface.write_fixture_checkpoints(str(d), n_lang=20)
    return str(d)


def test_interface_reports_clamped_and_empty_and_refuses_bad_segments(models_dir, monkeypatch):
    from ims_toucan_prosody_variance_amd import interface
    monkeypatch.setattr(interface, "MODELS_DIR", models_dir)
    monkeypatch.setenv("TOUCAN_PRECISION", "bf16")
    monkeypatch.delenv("TOUCAN_PY_SEQUENCER", raising=False)
    tts = interface.ToucanTTSInterface(device="cuda", tts_model_path="Meta", faster_vocoder=True)
    tts.set_language("en")
    assert tts.pipe is not None
    texts = [PHONES_20, PHONES_13, PHONES_20, PHONES_13]
    zs = [torch.from_numpy(syn.postflow_noise(70 + i, 4096)) for i in range(4)]
    plain = tts.synthesize_batch(texts, z_noise=zs)
    assert tts.last_prosody_fit is None
    base = [int(d.sum()) for d in tts.last_durations]
    fits = [Fit(target_frames=1 << 20), Fit(target_frames=1, bounds=(0.5, 2.0)), Fit(target_frames=base[2] + 5, bounds=(1.0, 1.0)), None]
    waves = tts.synthesize_batch(texts, z_noise=zs, prosody_fit=fits, pitch_variance_scale=[1.0, 1.0, 1.0, 1.0])
    fit = tts.last_prosody_fit
    status = [int(r[0, 4]) for r in fit["report"][:3]]
    print("status", [prosody_fit.STATUS[s] for s in status], "scales", fit["scales"].tolist())
    assert [prosody_fit.STATUS[s] for s in status] == ["CLAMPED_HIGH", "CLAMPED_LOW", "EMPTY"]
    assert fit["scales"][:, 0].tolist() == [4.0, 0.5, 1.0, 1.0] and all(not e.any() for e in fit["extra"])
    assert fit["report"][2][0, 1] == fit["report"][2][0, 7] == base[2] and fit["report"][3].shape == (0, 8)
    assert torch.equal(waves[2], plain[2]) and torch.equal(waves[3], plain[3])  # (bf16: whatever the batch)
    assert tts.last_prosody_stats is not None and tts.last_prosody_stats[1][3, 6] == base[3]
    one = tts(PHONES_13, input_is_phones=True, z_noise=zs[1], prosody_fit=Fit(target_seconds=(base[1] + 7) / 62.5))
    assert one.numel() // 384 in (base[1] + 7, base[1] + 6) and int(tts.last_durations[0].sum()) == base[1] + 7  # (the flow drops an odd last frame)
    # argument errors of the stage entry: the batch in flight keeps its durations, nothing was enqueued
    lib, h, st = tts.pipe.lib, tts.pipe.h, torch.cuda.current_stream().cuda_stream
    L = int(tts.last_durations[0].shape[0])
    d0 = torch.empty(L, dtype=torch.int32, device="cuda")
    p0, e0 = torch.empty(L, device="cuda"), torch.empty(L, device="cuda")
    capi.check(lib.tts_copy_prosody(h, d0.data_ptr(), p0.data_ptr(), e0.data_ptr(), st), "tts_copy_prosody")
    bad = {
        b"overlap": [(0, 2, 0, 3, 5, 0.25, 4, 1), (0, 2, 2, 4, 5, 0.25, 4, 1)],
        b"utterance 0, segment 0: the target": [(0, 0, 0, L, 0, 0.25, 4, 1)],
        b"utterance 0, segment 0: bounds": [(0, 0, 0, L, 5, 0.0, 4, 1)],
        b"utterance 0, segment 0: kind 0 takes the whole utterance": [(0, 0, 0, L - 1, 5, 0.25, 4, 1)],
        b"utterance 0, segment 1: a whole-utterance segment stands alone": [(0, 2, 0, 2, 5, 0.25, 4, 1), (0, 1, 0, L, 5, 0.0, 4, 1)],
        b"segment 0: utterance 1": [(1, 0, 0, L, 5, 0.25, 4, 1)],
        b"utterance 0, segment 0: rows": [(0, 2, 3, 3, 5, 0.25, 4, 1)],
    }
    frames = (ctypes.c_int32 * 1)()
    for message, rows in bad.items():
        seg = np.float32(rows)
        rc = lib.tts_control_and_regulate_t(h, None, None, None, 0, seg.ctypes.data_as(ctypes.c_void_p), len(rows), frames, st)
        assert rc != 0 and message in lib.tts_last_error(), (message, lib.tts_last_error())
    assert lib.tts_control_and_regulate_t(h, None, None, None, 0, None, 0, frames, st) != 0 and b"tts_control_and_regulate_c" in lib.tts_last_error()
    d1 = torch.empty_like(d0)
    capi.check(lib.tts_copy_prosody(h, d1.data_ptr(), p0.data_ptr(), e0.data_ptr(), st), "tts_copy_prosody")
    torch.cuda.synchronize()
    assert torch.equal(d0, d1)
