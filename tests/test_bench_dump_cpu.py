"""bench.py --dump-outputs on host tensors: what a caller receives, utterance by utterance, and the 64 MB bound."""
import os

import numpy as np
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd.ragged import Ragged
import bench


def _step_output(frames, phones):
    """A timed step's result in the form forward() returns it: packed tensors with alignment rows between utterances."""
    rag_mel, rag_p = Ragged(frames, "cpu", align=2), Ragged(phones, "cpu")
    mel_packed = torch.full((rag_mel.total_rows, 80), float("nan"))
    wav = torch.full((384 * rag_mel.total_rows,), float("nan"))
    for u, (b0, n) in enumerate(zip(rag_mel.begins, rag_mel.lengths)):
        mel_packed[b0:b0 + n] = u + torch.arange(n, dtype=torch.float32)[:, None] / 1e4
        wav[384 * b0:384 * (b0 + n)] = u + torch.arange(384 * n, dtype=torch.float32) / 1e7
    d = torch.arange(rag_p.total_rows, dtype=torch.int32)
    out = dict(rag_mel=rag_mel, mel=[mel_packed[b0:b0 + n] for b0, n in zip(rag_mel.begins, rag_mel.lengths)])
    for key, src in (("durations", d), ("pitch", d.float() / 7), ("energy", d.float() / 9)):
        out[key] = [src[b0:b0 + n] for b0, n in zip(rag_p.begins, rag_p.lengths)]
    return out, wav


def test_outputs_leave_out_alignment_rows(tmp_path):
    frames, phones = [5, 8, 3], [4, 6, 2]
    host = bench.outputs_to_host(*_step_output(frames, phones))
    assert host["mel"].shape == (16, 80) and host["wav"].shape == (16 * 384,)
    assert all(np.isfinite(a).all() for a in host.values())
    assert host["frames_per_utterance"].tolist() == frames
    assert host["durations"].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]
    assert host["mel"][5, 0] == 1.0 and host["wav"][384 * 13] == 2.0  # first frame of utterances 1 and 2
    names = bench.dump_outputs(str(tmp_path / "out"), host)
    assert names == ["durations", "energy", "frames_per_utterance", "mel", "pitch", "wav"]
    for name in names:
        a = np.load(tmp_path / "out" / f"{name}.npy")
        assert a.dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(a, host[name])


def test_large_outputs_keep_one_seeded_sample_of_frames(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 20)
    host = bench.outputs_to_host(*_step_output([300, 301, 299, 400], [60, 60, 60, 80]))
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), host)
    files = sorted(os.listdir(tmp_path / "a"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 1 << 20
    rows = np.load(tmp_path / "a" / "sampled_frames.npy")
    assert rows.dtype == np.float64 and np.all(np.diff(rows) > 0) and rows[-1] < 1300
    r = rows.astype(np.int64)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "mel.npy"), host["mel"][r])
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "wav.npy"), host["wav"].reshape(-1, 384)[r].reshape(-1))
    for f in files:  # the same sample on every run
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
