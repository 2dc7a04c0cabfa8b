"""numpy restatement of the scorer's kernels (csrc/score.hip), for the CPU tests and the golden maker.

* ``log_softmax32``: the fp32 log-softmax of the reference's ``pred.log_softmax(2)``, formed as (x - max) - log(sum exp(x - max)).
* ``ctc_nll``: the CTC forward variables over the extended label sequence in float64 (what tts_ctc_loss carries), with the skip
  transition into a label that differs from the label two states back; ``ctc_loss`` adds reduction "mean" at batch 1 and
  zero_infinity (Aligner.py:60,107).
* ``tts_losses``: the four losses of ToucanTTSLoss at batch 1 (ToucanTTSLoss.py:20-66), summed in float64.
"""
import numpy as np


def log_softmax32(logits):
    x = np.asarray(logits, dtype=np.float32)
    m = x.max(axis=1, keepdims=True)
    s = np.exp(x - m).sum(axis=1, keepdims=True, dtype=np.float32)
    return ((x - m) - np.log(s)).astype(np.float32)


def _lse(*xs):
    m = np.maximum.reduce(xs)
    out = np.full_like(m, -np.inf)
    ok = m > -np.inf
    acc = np.zeros_like(m)
    for x in xs:
        acc[ok] += np.exp(x[ok] - m[ok])
    out[ok] = m[ok] + np.log(acc[ok])
    return out


def ctc_nll(logp, targets, blank=144):
    """-log p(targets | frames) for log-probabilities logp [T, V] (float64 arithmetic); +inf when no alignment exists."""
    lp = np.asarray(logp, dtype=np.float64)
    tg = [int(t) for t in targets]
    S = 2 * len(tg) + 1
    lab = np.full(S, blank, dtype=np.int64)
    lab[1::2] = tg
    skip = np.zeros(S, dtype=bool)
    for s in range(3, S, 2):
        skip[s] = lab[s] != lab[s - 2]
    alpha = np.full(S, -np.inf)
    alpha[0] = lp[0, lab[0]]
    if S > 1:
        alpha[1] = lp[0, lab[1]]
    for t in range(1, lp.shape[0]):
        a1 = np.concatenate([[-np.inf], alpha])[:S]
        a2 = np.where(skip, np.concatenate([[-np.inf, -np.inf], alpha])[:S], -np.inf)
        alpha = _lse(alpha, a1, a2) + lp[t, lab]
    ll = _lse(alpha[S - 1:S], alpha[S - 2:S - 1])[0] if S > 1 else alpha[0]
    return -ll


def ctc_loss(logp, targets, blank=144):
    """CTCLoss(blank, zero_infinity=True) with reduction "mean" at batch 1: nll / max(n, 1), an infeasible alignment gives 0."""
    nll = ctc_nll(logp, targets, blank)
    return 0.0 if np.isinf(nll) else nll / max(len(targets), 1)


def tts_losses(before, after, gold, log_dur, pitch, energy, gold_dur, gold_pitch, gold_energy):
    """(l1, duration, pitch, energy) of one utterance: fp32 element differences, float64 sums."""
    f = lambda a: np.asarray(a, dtype=np.float32)
    before, after, gold = f(before), f(after), f(gold)
    T = gold.shape[0]
    l1 = (np.abs(before - gold).astype(np.float64).sum() + np.abs(after - gold).astype(np.float64).sum()) / (T * 80.0)
    target = np.log(np.asarray(gold_dur, dtype=np.float64) + 1.0).astype(np.float32)  # log(d + offset), offset 1.0
    d = (f(log_dur).reshape(-1) - target).astype(np.float64)
    p = (f(pitch).reshape(-1) - f(gold_pitch).reshape(-1)).astype(np.float64)
    e = (f(energy).reshape(-1) - f(gold_energy).reshape(-1)).astype(np.float64)
    return np.array([l1, (d * d).mean(), (p * p).mean(), (e * e).mean()])
