"""TEST INFRASTRUCTURE ONLY: the yardstick of the aligner's on-line fine-tuning (UtteranceCloner.py:75-94, Aligner.py:18-75) - the whole
procedure and each kernel's mathematics restated with torch CPU autograd on plain torch.nn.functional ops, in the dtype the caller
names (float64: the yardstick; float32: the same arithmetic rounded, whose distance from float64 sizes the tolerances).
tests/golden/make_finetune_golden.py asserts that ``fine_tune`` reproduces the reference's own loop.

Parameters are reference-schema state dicts (``convs.{0,2,..}.conv.weight`` ..., ``rnn.weight_ih_l0`` ..., ``proj.weight``).
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS, MOMENTUM, BLANK, LR, MAX_NORM = 1e-5, 0.1, 144, 0.1, 1.0
PARAM_KEYS = [f"convs.{2 * i}.{k}" for i in range(5) for k in ("conv.weight", "bnorm.weight", "bnorm.bias")] + \
             [f"rnn.{k}_l0{s}" for s in ("", "_reverse") for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")] + ["proj.weight", "proj.bias"]
STAT_KEYS = [f"convs.{2 * i}.bnorm.{k}" for i in range(5) for k in ("running_mean", "running_var")]


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype).clone()


def lstm_loop(xproj, w_hh, H):
    """The recurrence of one direction pair given the input projection with both biases [T, 8H] (columns [direction][i, f, g, o][H])
    and w_hh [2][4H, H] -> y [T, 2H]; differentiable, so xproj.grad is the gradient of the pre-activation gates."""
    T = xproj.shape[0]
    ys = []
    for d in range(2):
        h, c = xproj.new_zeros(H), xproj.new_zeros(H)
        out = [None] * T
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            g = xproj[t, d * 4 * H:(d + 1) * 4 * H] + w_hh[d] @ h
            i, f, gg, o = torch.sigmoid(g[:H]), torch.sigmoid(g[H:2 * H]), torch.tanh(g[2 * H:3 * H]), torch.sigmoid(g[3 * H:])
            c = f * c + i * gg
            h = o * torch.tanh(c)
            out[t] = h
        ys.append(torch.stack(out))
    return torch.cat(ys, dim=1)


def forward(P, S, mel, masks=None):
    """Aligner.forward at batch 1: training mode with the step's five keep-masks (running statistics S updated in place), or eval
    mode without.  P / S: dicts of tensors; mel [T, 80] -> logits [T, 145]."""
    x = mel.t()[None]  # [1, 80, T]
    for i in range(5):
        c = f"convs.{2 * i}."
        x = F.relu(F.conv1d(x, P[c + "conv.weight"], padding=1))
        x = F.batch_norm(x, S[c + "bnorm.running_mean"], S[c + "bnorm.running_var"], P[c + "bnorm.weight"], P[c + "bnorm.bias"],
                         training=masks is not None, momentum=MOMENTUM, eps=EPS)
        if masks is not None:
            x = x * torch.as_tensor(np.asarray(masks[i]), dtype=x.dtype).t()[None] * 2.0
    x = x[0].t()  # [T, 512]
    H = P["rnn.weight_hh_l0"].shape[1]
    xproj = torch.cat([x @ P["rnn.weight_ih_l0" + s].t() + P["rnn.bias_ih_l0" + s] + P["rnn.bias_hh_l0" + s] for s in ("", "_reverse")], dim=1)
    y = lstm_loop(xproj, [P["rnn.weight_hh_l0"], P["rnn.weight_hh_l0_reverse"]], H)
    return y @ P["proj.weight"].t() + P["proj.bias"]


def ctc(logits, ids):
    """CTCLoss(blank=144, zero_infinity=True), reduction "mean", of log_softmax(logits) at batch 1."""
    T = logits.shape[0]
    return F.ctc_loss(logits[:, None, :].log_softmax(2), torch.as_tensor(np.asarray(ids), dtype=torch.long)[None], torch.tensor([T]),
                      torch.tensor([len(ids)]), blank=BLANK, reduction="mean", zero_infinity=True)


def fine_tune(sd, mel, ids, masks, dtype=torch.float64, steps=5):
    """The five steps and the eval-mode logits after them.  -> dict: logits [T, 145], loss / norm [steps], the final state dict
    (parameters and running statistics) as numpy arrays."""
    P = {k: _t(sd[k], dtype).requires_grad_(True) for k in PARAM_KEYS}
    S = {k: _t(sd[k], dtype) for k in STAT_KEYS}
    mel = _t(mel, dtype)
    losses, norms = [], []
    for step in range(steps):
        loss = ctc(forward(P, S, mel, masks[step]), ids)
        grads = torch.autograd.grad(loss, [P[k] for k in PARAM_KEYS])
        total = torch.sqrt(sum((g * g).sum() for g in grads))
        coef = torch.clamp(MAX_NORM / (total + 1e-6), max=1.0)
        with torch.no_grad():
            for k, g in zip(PARAM_KEYS, grads):
                P[k] -= LR * (g * coef)
        losses.append(float(loss.detach()))
        norms.append(float(total))
    with torch.no_grad():
        logits = forward(P, S, mel, None)
    out = {k: v.detach().numpy() for k, v in P.items()}
    out.update({k: v.numpy() for k, v in S.items()})
    return {"logits": logits.numpy(), "loss": np.array(losses), "norm": np.array(norms), "state": out}


# ---- each kernel's mathematics ------------------------------------------------------------------------------------------------
def bn_train(z, gamma, beta, mask, rm, rv, dy, dtype=torch.float64):
    """tts_bn_train_forward / _backward: z [T, C] pre-ReLU -> dict(y, mean, istd, rm, rv, dz, dgamma, dbeta) by autograd."""
    z, gamma, beta = (_t(a, dtype).requires_grad_(True) for a in (z, gamma, beta))
    rm, rv = _t(rm, dtype), _t(rv, dtype)
    r = F.relu(z)
    y = F.batch_norm(r.t()[None], rm, rv, gamma, beta, training=True, momentum=MOMENTUM, eps=EPS)[0].t()
    if mask is not None:
        y = y * _t(mask, dtype) * 2.0
    dz, dg, db = torch.autograd.grad(y, [z, gamma, beta], _t(dy, dtype))
    mean, var = r.mean(0), r.var(0, unbiased=False)
    return {"y": y.detach().numpy(), "mean": mean.detach().numpy(), "istd": (1.0 / torch.sqrt(var + EPS)).detach().numpy(), "rm": rm.numpy(),
            "rv": rv.numpy(), "dz": dz.numpy(), "dgamma": dg.numpy(), "dbeta": db.numpy()}


def lstm_bptt(x, w_ih, w_hh, b_ih, b_hh, dy, dtype=torch.float64):
    """torch.nn.LSTM(C, H, bidirectional=True) on x [T, C] with weights [2][...] and the gradient dy of its output, by autograd:
    y, dx, dw_ih, dw_hh, db_ih, db_hh from the module; dgates [T, 8H] (the gradient of the pre-activation gates, which the module
    does not expose) from ``lstm_loop`` on the same numbers."""
    H, C = np.asarray(w_hh).shape[2], np.asarray(x).shape[1]
    lstm = torch.nn.LSTM(C, H, batch_first=True, bidirectional=True).to(dtype)
    with torch.no_grad():
        for d, s in enumerate(("", "_reverse")):
            for name, a in (("weight_ih", w_ih), ("weight_hh", w_hh), ("bias_ih", b_ih), ("bias_hh", b_hh)):
                getattr(lstm, f"{name}_l0{s}").copy_(_t(np.asarray(a)[d], dtype))
    xt = _t(x, dtype).requires_grad_(True)
    y = lstm(xt[None])[0][0]
    names = [f"{n}_l0{s}" for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh") for s in ("", "_reverse")]
    g = torch.autograd.grad(y, [xt] + [getattr(lstm, n) for n in names], _t(dy, dtype))
    pair = lambda k: np.stack([g[1 + 2 * k].numpy(), g[2 + 2 * k].numpy()])
    xproj = torch.cat([_t(x, dtype) @ _t(np.asarray(w_ih)[d], dtype).t() + _t(np.asarray(b_ih)[d], dtype) + _t(np.asarray(b_hh)[d], dtype)
                       for d in range(2)], dim=1).requires_grad_(True)
    y2 = lstm_loop(xproj, [_t(np.asarray(w_hh)[d], dtype) for d in range(2)], H)
    dgates, = torch.autograd.grad(y2, [xproj], _t(dy, dtype))
    return {"y": y.detach().numpy(), "y_loop": y2.detach().numpy(), "dx": g[0].numpy(), "dw_ih": pair(0), "dw_hh": pair(1), "db_ih": pair(2),
            "db_hh": pair(3), "dgates": dgates.numpy()}


def ctc_grad(logits, ids, dtype=torch.float64):
    """-> (loss, d loss / d logits [T, 145]) by autograd through log_softmax and F.ctc_loss."""
    lg = _t(logits, dtype).requires_grad_(True)
    loss = ctc(lg, ids)
    g, = torch.autograd.grad(loss, [lg])
    return float(loss.detach()), g.numpy()


def clip_update(theta, grad, dtype=torch.float64):
    """-> (norm, updated theta): clip_grad_norm_(1.0) then SGD(lr 0.1)."""
    p, g = _t(theta, dtype), _t(grad, dtype)
    total = torch.sqrt((g * g).sum())
    coef = torch.clamp(MAX_NORM / (total + 1e-6), max=1.0)
    return float(total), (p - LR * (g * coef)).numpy()
