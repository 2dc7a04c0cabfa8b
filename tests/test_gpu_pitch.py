"""The pitch tracker's kernels (csrc/pitch.hip) on the MI355X against the float64 restatement in tests/pitch_ref.py: the candidates of
every frame, the path kernel fed the restatement's candidates (both forms of its back-pointer store), the tracker end to end, a
ragged batch against its utterances one by one, and the cloner's ``f0="track"`` / ``track_pitch=True``."""
import os

import numpy as np
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import capi, fixture_weights as fw, pitch, style
from tests import pitch_ref as pr

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL = pr.SHORT + ("long40",)

# Bounds: 4 x the worst error measured on these signals on the MI355X (DESIGN.md section 12 records the measurement): |r - ref|,
# relative frequency error and strength error of the candidates on the frames that are not fragile.
MEASURED_R, MEASURED_FREQ, MEASURED_STRENGTH = 1.546e-6, 2.892e-6, 1.537e-6
FREQ_RTOL = 4 * MEASURED_FREQ
STRENGTH_ATOL = 4 * MEASURED_STRENGTH
R_ATOL = 4 * MEASURED_R


def wave(name):
    return pr.long40()[0] if name == "long40" else pr.signals()[name][0]


@pytest.fixture(scope="module")
def tracker():
    return pitch.PitchTracker(DEV)


@pytest.fixture(scope="module")
def batch(tracker):
    """Every signal in one ragged batch, run once: (layout, candidates on the host, f0 per signal)."""
    lay = tracker.layout([wave(n) for n in ALL])
    freq, strength, n_cand, r = tracker.candidates(lay, with_r=True)
    f0 = tracker.path(freq, strength, n_cand, lay["frames"]).cpu().numpy()
    host = {"freq": freq.cpu().numpy(), "strength": strength.cpu().numpy(), "n_cand": n_cand.cpu().numpy(), "r": r.cpu().numpy()}
    spans = {n: (b, b + T) for n, b, T in zip(ALL, lay["frame_begin"], lay["frames"])}
    return host, spans, f0


def test_candidates_against_the_restatement(batch):
    """On every frame that is not fragile the kernel finds the restatement's candidate set: the same number, lag by lag, each
    frequency and strength within the bound; the unvoiced candidate's strength too.  r itself is compared on every frame."""
    host, spans, _ = batch
    worst = {"r": 0.0, "freq": 0.0, "strength": 0.0}
    frames = fragile = 0
    for name in ALL:
        ref = pr.analysed(name)
        a, b = spans[name]
        assert b - a == len(ref["f0"]), name
        worst["r"] = max(worst["r"], float(np.abs(host["r"][a:b] - ref["r"]).max()))
        ok = ~ref["fragile"]
        frames, fragile = frames + len(ok), fragile + int((~ok).sum())
        assert np.array_equal(host["n_cand"][a:b][ok], ref["n_cand"][ok]), name
        got_f, got_s = host["freq"][a:b][ok], host["strength"][a:b][ok]
        ref_f, ref_s = ref["freq"][ok], ref["strength"][ok]
        used = np.arange(pr.MAX_CAND)[None, :] < ref["n_cand"][ok][:, None]
        assert not got_f[~used].any() and not got_s[~used].any() and not got_f[:, 0].any(), name
        voiced = used & (ref_f > 0)
        # same lag: 16000 / f within the refinement's bracket of one sample either side of the restatement's lag
        assert (np.abs(pr.SR / got_f[voiced] - ref["lag"][ok][voiced]) <= 1.0).all(), name
        worst["freq"] = max(worst["freq"], float((np.abs(got_f[voiced] - ref_f[voiced]) / ref_f[voiced]).max(initial=0.0)))
        worst["strength"] = max(worst["strength"], float(np.abs(got_s[used] - ref_s[used]).max()))
    print(f"candidates on {frames} frames ({fragile} fragile): worst |r - ref| {worst['r']:.3e}, worst relative frequency error "
          f"{worst['freq']:.3e}, worst strength error {worst['strength']:.3e}")
    assert worst["r"] <= R_ATOL and worst["freq"] <= FREQ_RTOL and worst["strength"] <= STRENGTH_ATOL


@pytest.mark.parametrize("force_scratch", [False, True])
def test_path_kernel_on_the_restatements_candidates(tracker, force_scratch):
    """Fed the restatement's candidates (as float32) the path kernel returns the restatement's path exactly: back-pointers in LDS
    for the short signals and in the scratch buffer for the 40 s one, then in the scratch buffer for all."""
    refs = [pr.analysed(n) for n in ALL]
    frames = [len(r["f0"]) for r in refs]
    assert max(frames) > capi.PITCH_PATH_LDS_FRAMES > sorted(frames)[-2] and min(frames) == 1
    freq = np.concatenate([r["freq"] for r in refs]).astype(np.float32)
    strength = np.concatenate([r["strength"] for r in refs]).astype(np.float32)
    n_cand = np.concatenate([r["n_cand"] for r in refs]).astype(np.int32)
    t = lambda a: torch.from_numpy(a).to(DEV)
    f0 = tracker.path(t(freq), t(strength), t(n_cand), frames, force_scratch=force_scratch).cpu().numpy()
    want = np.concatenate([r["f0"] for r in refs]).astype(np.float32)
    assert np.array_equal(f0, want)


def test_path_kernel_reports_what_it_cannot_lay_out(tracker):
    """A frame without candidates: the utterance's f0 is -1 and its neighbour is untouched by it."""
    ref = pr.analysed("glide1")
    T = len(ref["f0"])
    t = lambda a, dt: torch.from_numpy(np.concatenate([a, a]).astype(dt)).to(DEV)
    n_cand = np.concatenate([ref["n_cand"], ref["n_cand"]]).astype(np.int32)
    n_cand[3] = 0
    f0 = tracker.path(t(ref["freq"], np.float32), t(ref["strength"], np.float32), torch.from_numpy(n_cand).to(DEV), [T, T]).cpu().numpy()
    assert (f0[:T] == -1).all() and np.array_equal(f0[T:], ref["f0"].astype(np.float32))


def test_tracker_end_to_end(batch):
    """Voicing as the restatement's at every frame and voiced f0 within the bound; a frame may differ only where the restatement
    itself calls the decision close (path margin under 1e-4), and at most 1 % of the frames may."""
    _, spans, f0 = batch
    total = excused = 0
    worst = 0.0
    for name in ALL:
        ref = pr.analysed(name)
        a, b = spans[name]
        got, want = f0[a:b], ref["f0"]
        differs = (got > 0) != (want > 0)
        both = (got > 0) & (want > 0)
        rel = np.zeros(len(got))
        rel[both] = np.abs(got[both] - want[both]) / want[both]
        differs |= rel > FREQ_RTOL
        assert (ref["margin"][differs] < 1e-4).all(), (name, np.nonzero(differs)[0], rel.max())
        worst = max(worst, float(rel[~differs].max()))
        total, excused = total + len(got), excused + int(differs.sum())
    print(f"end to end on {total} frames: worst relative f0 error {worst:.3e}, {excused} excused")
    assert excused <= 0.01 * total


def test_batch_equals_utterances_alone(tracker, batch):
    """The ragged batch of all signals returns each track bit for bit as the signal alone does (and as track() does)."""
    _, spans, f0 = batch
    together = tracker.track([wave(n) for n in ALL])
    for name, trk in zip(ALL, together):
        a, b = spans[name]
        assert trk.dtype == np.float32 and np.array_equal(trk, f0[a:b]), name
        assert np.array_equal(tracker.track([wave(name)])[0], trk), name
    assert tracker.track([]) == []
    with pytest.raises(ValueError):
        tracker.track([np.zeros(pr.MIN_SAMPLES - 1, dtype=np.float32)])


def test_cloner_tracks_pitch_on_request(tmp_path, monkeypatch):
    """extract_prosody(f0="track") equals, bit for bit, feeding the device track of the same wave through f0=<array>; an instance
    made with track_pitch=True does that without the keyword; the default still returns no pitch."""
    from ims_toucan_prosody_variance_amd import interface
    models = tmp_path / "Models"
    interface.write_fixture_checkpoints(str(models), n_lang=20)
    interface.write_fixture_aligner_checkpoint(str(models))
    monkeypatch.setattr(interface, "MODELS_DIR", str(models))
    from InferenceInterfaces.UtteranceCloner import UtteranceCloner
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aligner", "aligner.npz"))
    phones = [str(G["clone_phones"][u]) for u in (0, 1)]
    recordings = [pr.glide(31 + u, seconds=int(G[f"clone{u}_samples"]) / 16000.0)[0] for u in (0, 1)]
    ref_wav = str(tmp_path / "ref.wav")
    interface.write_wav(ref_wav, recordings[1], 16000)
    recordings[1] = style.read_audio(ref_wav)[0]  # as the file holds it (16-bit)
    model = str(models / "ToucanTTS_Meta" / "best.pt")
    cl = UtteranceCloner(model_id=model, device=DEV, language="en")
    assert cl.extract_prosody(phones[1], ref_wav, lang="en")[1] is None
    same = lambda x, y: all(torch.equal(a, b) for a, b in zip(x[:3], y[:3])) and tuple(x[3:]) == tuple(y[3:])
    wave16 = style.normalize_reference_audio(style.read_audio(ref_wav)[0], 16000)
    track = pitch.PitchTracker(DEV).track([wave16])[0]
    assert (track > 0).sum() > len(track) // 2
    tracked = cl.extract_prosody(phones[1], ref_wav, lang="en", f0="track")
    assert tracked[1] is not None and bool(torch.isfinite(tracked[1]).all()) and float(tracked[1].max()) > 0
    assert same(tracked, cl.extract_prosody(phones[1], ref_wav, lang="en", f0=track))
    # a batch may mix a given track, the tracker and (in another call) nothing
    norm0 = style.normalize_reference_audio(recordings[0], 16000)
    mixed = cl.extract_prosody_batch(phones, recordings, 16000, f0=[pitch.PitchTracker(DEV).track([norm0])[0], "track"])
    assert same(mixed[1], tracked) and same(mixed[0], cl.extract_prosody_batch(phones[:1], recordings[:1], 16000, f0="track")[0])
    assert cl.extract_prosody_batch(phones, recordings, 16000)[1][1] is None
    z = torch.from_numpy(fw.normal("clone.z", (80, int(tracked[0].sum())), 1, 0.8))
    cloned = cl.clone_utterance(ref_wav, ref_wav, phones[1], lang="en", f0="track", z_noise=z)
    plain = cl.tts(phones[1], durations=tracked[0], pitch=tracked[1], energy=tracked[2], input_is_phones=True, z_noise=z).cpu().numpy()
    assert np.array_equal(cloned, plain)
    angel = cl.biblical_accurate_angel_mode(ref_wav, phones[1], [ref_wav, ref_wav], lang="en", f0="track", z_noise=[z, z])
    assert np.isfinite(angel).all() and len(angel) > 0
    tracking = UtteranceCloner(model_id=model, device=DEV, language="en", track_pitch=True)
    assert same(tracking.extract_prosody(phones[1], ref_wav, lang="en"), tracked)
    assert np.array_equal(tracking.clone_utterance(ref_wav, ref_wav, phones[1], lang="en", z_noise=z), cloned)
