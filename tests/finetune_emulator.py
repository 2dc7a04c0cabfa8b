"""TEST INFRASTRUCTURE ONLY: the aligner emulator (tests/aligner_emulator.py) extended by the entry points of include/toucan_train.h
(csrc/train.hip), so that finetune.py's sequencing - arenas, padded activations, overlapping-row products, per-step recurrences,
clip and update - runs end to end on CPU tensors.  Each entry is the closed form the kernel implements, in float64 numpy on the
float32 buffers: written out by hand, so that its agreement with the autograd yardstick (tests/finetune_ref.py) checks both."""
import ctypes as C

import numpy as np

from ims_toucan_prosody_variance_amd import capi
from tests.abi_emulator import _arr, _mat
from tests.aligner_emulator import AlignerEmulator


def _bytes(ptr, n):
    return np.ctypeslib.as_array((C.c_uint8 * int(n)).from_address(int(ptr)))


def _f64(ptr, n):
    return np.ctypeslib.as_array((C.c_double * int(n)).from_address(int(ptr)))


def _view(ptr, rows, cols, ld):
    """[rows, cols] float64 copy of a strided float32 operand whose rows may overlap."""
    return np.array(_mat(ptr, rows, cols, ld), dtype=np.float64)


def _lse(*xs):
    m = max(xs)
    return m if m == -np.inf else m + np.log(sum(np.exp(x - m) for x in xs))


def ctc_from_log_probs(LP, targets, blank):
    """CTC loss (zero_infinity, / n) and its gradient with respect to the logits, from the frames' log-probabilities [T, n_symbols]:
    forward and backward variables over the 2n+1 extended states in float64, a frame row at a time.  -> (loss, grad float64)."""
    LP, tg = np.asarray(LP, dtype=np.float64), np.asarray(targets)
    t, n = LP.shape[0], len(tg)
    S = 2 * n + 1
    lab = np.full(S, blank)
    lab[1::2] = tg
    skip = np.zeros(S, dtype=bool)  # the transition s - 2 -> s: into a label that differs from the label two states back
    skip[3::2] = tg[1:] != tg[:-1]
    ninf = lambda k: np.full(k, -np.inf)
    a, b = np.full((t, S), -np.inf), np.full((t, S), -np.inf)
    a[0, :2] = LP[0, lab[:2]]
    for i in range(1, t):
        p = a[i - 1]
        two = np.where(skip, np.concatenate([ninf(2), p[:-2]]), -np.inf)
        a[i] = np.logaddexp(np.logaddexp(p, np.concatenate([ninf(1), p[:-1]])), two) + LP[i, lab]
    b[t - 1, S - 2:] = LP[t - 1, lab[S - 2:]]
    for i in range(t - 2, -1, -1):
        p = b[i + 1]
        two = np.where(np.concatenate([skip[2:], [False, False]]), np.concatenate([p[2:], ninf(2)]), -np.inf)
        b[i] = np.logaddexp(np.logaddexp(p, np.concatenate([p[1:], ninf(1)])), two) + LP[i, lab]
    ll = _lse(a[t - 1, S - 1], a[t - 1, S - 2])
    if ll == -np.inf:
        return 0.0, np.zeros_like(LP)
    with np.errstate(invalid="ignore"):
        p = np.exp(a + b - LP[:, lab] - ll)
    p[~np.isfinite(a + b)] = 0.0
    post = np.zeros_like(LP)
    for s in range(S):
        post[:, lab[s]] += p[:, s]
    return -ll / n, (np.exp(LP) - post) / n


class FineTuneEmulator(AlignerEmulator):
    def tts_gemm_f32(self, op, a, lda, b, ldb, c, ldc, bias, m, n, k, accumulate, stream):
        self._count("gemm_f32")
        if m == 0 or n == 0:
            return 0
        if k > 0:
            A = _view(a, k, m, lda).T if op == capi.GEMM_TN else _view(a, m, k, lda)
            B = _view(b, n, k, ldb).T if op == capi.GEMM_NT else _view(b, k, n, ldb)
            out = A @ B
        else:
            out = np.zeros((m, n))
        if bias:
            out = out + _arr(bias, n).astype(np.float64)[None]
        Cm = _mat(c, m, n, ldc)
        Cm[:] = (out + Cm if accumulate else out).astype(np.float32)
        return 0

    def _keep(self, mask, t, c):
        return _bytes(mask, t * c).reshape(t, c).astype(np.float64) * 2.0 if mask else np.ones((t, c))

    def tts_bn_train_forward(self, z, ldz, mask, gamma, beta, rm, rv, y, ldy, save_mean, save_istd, t, c, eps, momentum, stream):
        self._count("bn_train_forward")
        assert t >= 2 and c % 64 == 0
        r = np.maximum(_view(z, t, c, ldz), 0.0)
        mean = r.mean(0)
        ssd = ((r - mean) ** 2).sum(0)
        istd = 1.0 / np.sqrt(ssd / t + eps)
        out = ((r - mean) * istd * _arr(gamma, c) + _arr(beta, c)) * self._keep(mask, t, c)
        _mat(y, t, c, ldy)[:] = out.astype(np.float32)
        _arr(save_mean, c)[:] = mean
        _arr(save_istd, c)[:] = istd
        if rm:
            _arr(rm, c)[:] = (1.0 - momentum) * _arr(rm, c).astype(np.float64) + momentum * mean
        if rv:
            _arr(rv, c)[:] = (1.0 - momentum) * _arr(rv, c).astype(np.float64) + momentum * ssd / (t - 1)
        return 0

    def tts_bn_train_backward(self, dy, lddy, z, ldz, mask, gamma, save_mean, save_istd, dz, lddz, dgamma, dbeta, t, c, stream):
        self._count("bn_train_backward")
        Z = _view(z, t, c, ldz)
        mean, istd = _arr(save_mean, c).astype(np.float64), _arr(save_istd, c).astype(np.float64)
        g = _view(dy, t, c, lddy) * self._keep(mask, t, c)
        xh = (np.maximum(Z, 0.0) - mean) * istd
        s1, s2 = g.sum(0), (g * xh).sum(0)
        _mat(dz, t, c, lddz)[:] = np.where(Z > 0, _arr(gamma, c) * istd * (g - s1 / t - xh * s2 / t), 0.0).astype(np.float32)
        _arr(dbeta, c)[:] = s1
        _arr(dgamma, c)[:] = s2
        return 0

    def tts_bn_eval_affine(self, gamma, beta, rm, rv, scale, shift, c, eps, stream):
        self._count("bn_eval_affine")
        s = _arr(gamma, c).astype(np.float64) / np.sqrt(_arr(rv, c).astype(np.float64) + eps)
        _arr(scale, c)[:] = s
        _arr(shift, c)[:] = _arr(beta, c).astype(np.float64) - _arr(rm, c).astype(np.float64) * s
        return 0

    def tts_lstm_train_step(self, xproj, ldx, w_hh, b_ih, b_hh, y, ldy, gates, cseq, t, hidden, step, stream):
        self._count("lstm_train_step")
        H = hidden
        W = _arr(w_hh, 2 * 4 * H * H).reshape(2, 4 * H, H).astype(np.float64)
        bias = (_arr(b_ih, 8 * H).astype(np.float64) + _arr(b_hh, 8 * H)).reshape(2, 4 * H)
        Y, G, Cs = _mat(y, t, 2 * H, ldy), _arr(gates, t * 8 * H).reshape(t, 2, 4 * H), _arr(cseq, t * 2 * H).reshape(t, 2, H)
        sig = lambda v: 1.0 / (1.0 + np.exp(-v))
        for d in range(2):
            row, prev = (step, step - 1) if d == 0 else (t - 1 - step, t - step)
            h = Y[prev, d * H:(d + 1) * H].astype(np.float64) if step > 0 else np.zeros(H)
            cp = Cs[prev, d].astype(np.float64) if step > 0 else np.zeros(H)
            g = _mat(xproj, t, 8 * H, ldx)[row, d * 4 * H:(d + 1) * 4 * H].astype(np.float64) + bias[d] + W[d] @ h
            i, f, gg, o = sig(g[:H]), sig(g[H:2 * H]), np.tanh(g[2 * H:3 * H]), sig(g[3 * H:])
            c = f * cp + i * gg
            G[row, d] = np.concatenate([i, f, gg, o])
            Cs[row, d] = c
            Y[row, d * H:(d + 1) * H] = o * np.tanh(c)
        return 0

    def tts_lstm_backward_step(self, dy, lddy, w_hh, gates, cseq, dgates, dc, t, hidden, step, stream):
        self._count("lstm_backward_step")
        H = hidden
        W = _arr(w_hh, 2 * 4 * H * H).reshape(2, 4 * H, H).astype(np.float64)
        G, Cs = _arr(gates, t * 8 * H).reshape(t, 2, 4 * H).astype(np.float64), _arr(cseq, t * 2 * H).reshape(t, 2, H).astype(np.float64)
        DG, DC = _arr(dgates, t * 8 * H).reshape(t, 2, 4 * H), _arr(dc, 2 * H).reshape(2, H)
        for d in range(2):
            row, nxt, prev = (step, step + 1, step - 1) if d == 0 else (t - 1 - step, t - 2 - step, t - step)
            dh = _mat(dy, t, 2 * H, lddy)[row, d * H:(d + 1) * H].astype(np.float64)
            dcv = np.zeros(H)
            if step < t - 1:
                dh = dh + W[d].T @ DG[nxt, d].astype(np.float64)
                dcv = DC[d].astype(np.float64)
            i, f, gg, o = G[row, d, :H], G[row, d, H:2 * H], G[row, d, 2 * H:3 * H], G[row, d, 3 * H:]
            cp = Cs[prev, d] if step > 0 else np.zeros(H)
            tc = np.tanh(Cs[row, d])
            dcv = dcv + dh * o * (1.0 - tc * tc)
            DG[row, d] = np.concatenate([dcv * gg * i * (1 - i), dcv * cp * f * (1 - f), dcv * i * (1 - gg * gg), dh * tc * o * (1 - o)])
            DC[d] = dcv * f
        return 0

    def tts_ctc_grad(self, logits, ld, n_symbols, t, targets, n_targets, blank, alpha, lp, loss, grad, ldg, stream):
        self._count("ctc_grad")
        X = _mat(logits, t, n_symbols, ld).astype(np.float32)
        m = X.max(1, keepdims=True)
        LP = (X - m) - np.log(np.exp(X - m).sum(1, keepdims=True, dtype=np.float32))  # the fp32 log_softmax
        _mat(lp, t, n_symbols, n_symbols)[:] = LP
        value, g = ctc_from_log_probs(LP, _arr(targets, n_targets, np.int32), blank)
        _arr(loss, 1)[0] = value
        _mat(grad, t, n_symbols, ldg)[:] = g.astype(np.float32)
        return 0

    def tts_col_sum(self, x, ldx, rows, cols, out, out2, stream):
        self._count("col_sum")
        s = _view(x, rows, cols, ldx).sum(0)
        _arr(out, cols)[:] = s
        if out2:
            _arr(out2, cols)[:] = s
        return 0

    def tts_sumsq(self, x, n, partials, norm, stream):
        self._count("sumsq")
        _arr(norm, 1)[0] = np.sqrt((_arr(x, n).astype(np.float64) ** 2).sum())
        return 0

    def tts_sgd_clip_update(self, p, g, n, norm, max_norm, lr, stream):
        self._count("sgd_clip_update")
        coef = min(1.0, max_norm / (float(_arr(norm, 1)[0]) + 1e-6))
        P = _arr(p, n)
        P[:] = (P.astype(np.float64) - lr * (_arr(g, n).astype(np.float64) * coef)).astype(np.float32)
        return 0


def install(monkeypatch):
    emu = FineTuneEmulator()
    monkeypatch.setattr(capi, "_LIB", emu)
    return emu
