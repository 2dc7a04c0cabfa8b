"""TEST INFRASTRUCTURE ONLY: numpy / torch-CPU restatement of the prosody cloner's extraction path - the oracle the aligner goldens
pin (tests/golden/make_aligner_golden.py asserts that it reproduces the reference) and the GPU kernels are compared with.

* ``mas`` - binarize_alignment (Aligner.py:202-234) + DurationCalculator in float32 numpy, row-vectorised with the reference's
  per-cell operations, plus the smallest decision margin along the chosen path;
* ``postprocess`` - zeros at word boundaries, the 3/5 - 2/5 repair of repeated phonemes (UtteranceCloner.py:95-131);
* ``token_average`` - EnergyCalculator / PitchCalculator._average_by_duration and their norm_by_average, in torch float32;
* ``aligner_logits`` - the Aligner's forward from ``align.pack_aligner``'s folded weights through torch.nn on the CPU.
"""
import numpy as np
import torch
import torch.nn.functional as F


def mas(pred_max, log64=False):
    """pred_max float32 [T, L] -> (durations int64 [L], smallest |left - stay| along the path, that margin in ulps of the scores).
    log64: the logarithm correctly rounded to float32 (what tts_mas_durations computes) instead of numpy's float32 log, which is up
    to 3 ulps off; every other operation is the same, so with log64 the kernel's decisions are reproduced bit for bit."""
    p = np.asarray(pred_max, dtype=np.float32)
    T, L = p.shape
    x = p + (np.abs(p).max() + 1.0)  # same expression and dtypes as Aligner.py:208-210
    attn = np.log(x.astype(np.float64)).astype(np.float32) if log64 else np.log(x)
    attn[0, 1:] = -np.inf
    lp = np.zeros_like(attn)
    lp[0] = attn[0]
    take = np.zeros((T, L), dtype=bool)
    for i in range(1, T):
        prev = lp[i - 1]
        t = np.zeros(L, dtype=bool)
        t[1:] = prev[:-1] >= prev[1:]
        left = np.concatenate([prev[:1], prev[:-1]])
        lp[i] = attn[i] + np.where(t, left, prev)
        take[i] = t
    dur = np.zeros(L, dtype=np.int64)
    curr, margin, ulps = L - 1, np.inf, np.inf
    for i in range(T - 1, 0, -1):
        dur[curr] += 1
        if curr >= 1:
            a, b = lp[i - 1, curr - 1], lp[i - 1, curr]
            if np.isfinite(a) and np.isfinite(b):
                m = float(abs(np.float64(a) - np.float64(b)))
                margin = min(margin, m)
                ulps = min(ulps, m / float(np.spacing(np.float32(max(abs(a), abs(b))))))
        curr -= int(take[i, curr])
    dur[0] += 1  # opt[0, 0] = 1 after the walk; argmax takes the first 1
    return dur, margin, ulps


def mas_float64_score(pred_max, dur):
    """Float64 score of the monotonic path that gives `dur` (frame 0 on token 0) - to judge whether two duration vectors are a near tie."""
    p = np.asarray(pred_max, dtype=np.float64)
    a = np.log(p + (np.abs(p).max() + 1.0))
    j = np.repeat(np.arange(len(dur)), dur)
    return float(a[np.arange(len(j)), j].sum())


def flags_of(feats):
    """bit 0: word boundary; bit 1: the feature vector equals the previous one."""
    feats = np.asarray(feats)
    f = np.zeros(len(feats), dtype=np.int32)
    for k in range(len(feats)):
        if feats[k][21] != 0:
            f[k] |= 1
        if k > 0 and np.array_equal(feats[k], feats[k - 1]):
            f[k] |= 2
    return f


def postprocess(dur_nb, flags):
    dur = torch.as_tensor(np.asarray(dur_nb, dtype=np.int64))
    for k in np.nonzero(np.asarray(flags) & 1)[0]:
        dur = torch.cat([dur[:k], torch.LongTensor([0]), dur[k:]])
    for k in range(1, len(flags)):
        if flags[k] & 2:
            total = dur[k - 1] + dur[k]
            n1 = int((total / 5) * 3)
            dur[k - 1] = n1
            dur[k] = total - n1
    return dur.numpy()


def token_average(x, dur, keep, mode):
    """mode 0: energy (every frame), 1: pitch (frames > 0); keep == 0 zeroes a token; then / mean of the nonzero tokens."""
    x = torch.as_tensor(np.asarray(x, dtype=np.float32))
    d = torch.as_tensor(np.asarray(dur, dtype=np.int64))
    cum = F.pad(d.cumsum(dim=0), (1, 0))
    out = []
    for k, (s, e) in enumerate(zip(cum[:-1], cum[1:])):
        seg = x[s:e]
        if mode == 1:
            seg = seg.masked_select(seg.gt(0.0))
        v = seg.mean() if len(seg) != 0 else x.new_tensor(0.0)
        out.append(v if keep[k] else torch.tensor(0.0))
    out = torch.stack(out)
    return (out / out[out != 0.0].mean()).numpy()


def frame_energy(spec, bins):
    s = np.asarray(spec, dtype=np.float64)
    return np.sqrt(np.maximum((s[:, :bins] ** 2 + s[:, bins:2 * bins] ** 2).sum(1), 1e-10))


def adjust_centered(x, n):
    x = torch.as_tensor(np.asarray(x, dtype=np.float32))
    if n > len(x):
        x = F.pad(x, (int(np.ceil((n - len(x)) / 2)), (n - len(x)) // 2))
    return x[:n].numpy()


@torch.no_grad()
def aligner_logits(packed, mel):
    """The Aligner's forward (Aligner.py:62-72, batch 1) from pack_aligner's folded arrays: conv, ReLU, BatchNorm as scale / shift
    (layers 1-4); conv, ReLU (layer 5, its BatchNorm folded into the LSTM input weights); torch.nn.LSTM; Linear."""
    x = torch.as_tensor(np.asarray(mel, dtype=np.float32)).t()[None]  # [1, 80, T]
    for i in range(5):
        x = F.relu(F.conv1d(x, torch.from_numpy(packed["conv_w"][i]), padding=1))
        if i < 4:
            x = x * torch.from_numpy(packed["bn_scale"][i])[None, :, None] + torch.from_numpy(packed["bn_shift"][i])[None, :, None]
    H = packed["hidden"]
    lstm = torch.nn.LSTM(x.shape[1], H, batch_first=True, bidirectional=True)
    for d, suf in enumerate(("", "_reverse")):
        getattr(lstm, "weight_ih_l0" + suf).copy_(torch.from_numpy(packed["w_ih"][d]))
        getattr(lstm, "weight_hh_l0" + suf).copy_(torch.from_numpy(packed["w_hh_t"][d].T.copy()))
        getattr(lstm, "bias_ih_l0" + suf).copy_(torch.from_numpy(packed["b_ih"][d]))
        getattr(lstm, "bias_hh_l0" + suf).zero_()
    h, _ = lstm(x.transpose(1, 2))
    return F.linear(h, torch.from_numpy(packed["proj_w"]), torch.from_numpy(packed["proj_b"]))[0].numpy()


def lstm_reference(xproj, w_hh_t, lengths, H):
    """float64 recurrence of the bidirectional LSTM over a packed batch given its input projection [rows, 8H] (biases included)."""
    X = np.asarray(xproj, dtype=np.float64)
    W = np.asarray(w_hh_t, dtype=np.float64)
    y = np.zeros((X.shape[0], 2 * H))
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    b0 = 0
    for n in lengths:
        for d in range(2):
            h, c = np.zeros(H), np.zeros(H)
            order = range(n) if d == 0 else range(n - 1, -1, -1)
            for t in order:
                g = X[b0 + t, d * 4 * H:(d + 1) * 4 * H] + h @ W[d]
                i, f, gg, o = sig(g[:H]), sig(g[H:2 * H]), np.tanh(g[2 * H:3 * H]), sig(g[3 * H:])
                c = f * c + i * gg
                h = o * np.tanh(c)
                y[b0 + t, d * H:(d + 1) * H] = h
        b0 += n
    return y
