"""float64 numpy restatement of the PostFlow's forward pass and the glow loss (Glow.py:342-391 with infer=False, ToucanTTS.py:349-353),
from state-dict arrays with the weight norm folded (``fold_weight_norm`` here, in float64; packing.fold_weight_norm's fp32 weights
are what the kernels run on), for the CPU tests, the GPU tests and the golden maker
(tests/golden/make_glow_golden.py asserts that it reproduces the reference's float64 modules to 1e-10).  Everything is time-major:
mels [T, 80], squeezed rows [T // 2, 160] = [frame 2r | frame 2r + 1] (glow_utils.py:28-40; an odd last frame is dropped).

* ``rows_forward``: what tts_glow_forward_rows does to rows, in float64 from the arrays it is given.
* ``flow_forward``: the 18 blocks on a gold mel, conditioned on [refined mel | up-sampled text] -> z, per-row log-determinants.
* ``row_parts`` / ``loss_from_parts``: the two quantities per row that tts_glow_nll_reduce forms, and the loss from them.
"""
import numpy as np

N_BLOCKS, HALF_LOG_2PI = 18, 0.5 * np.log(2.0 * np.pi)
FLOW = "post_flow.flows."


def _f(a):
    return np.asarray(a, dtype=np.float64)


def fold_weight_norm(sd):
    """{..weight_g, ..weight_v} -> {..weight} without the rounding to fp32 of packing.fold_weight_norm: what the reference's modules
    cast to float64 compute.  Other entries pass through."""
    out = {}
    for k, v in sd.items():
        if k.endswith(".weight_g"):
            base = k[:-len(".weight_g")]
            vv = _f(sd[base + ".weight_v"])
            nrm = np.sqrt((vv.reshape(vv.shape[0], -1) ** 2).sum(axis=1)).reshape([-1] + [1] * (vv.ndim - 1))
            out[base + ".weight"] = vv * (_f(v) / nrm)
        elif not k.endswith(".weight_v"):
            out[k] = np.asarray(v)
    return out


def squeeze(x):
    x = _f(x)
    rs = x.shape[0] // 2
    return x[:2 * rs].reshape(rs, 2 * x.shape[1])


def conv1d(x, w, b):
    """x [T, cin], torch Conv1d weight [cout, cin, k] with zero 'same' padding (k odd, dilation 1) -> [T, cout]."""
    x, w = _f(x), _f(w)
    T, k = x.shape[0], w.shape[2]
    xp = np.pad(x, ((k // 2, k // 2), (0, 0)))
    y = np.zeros((T, w.shape[0]))
    for j in range(k):
        y += xp[j:j + T] @ w[:, :, j].T
    return y if b is None else y + _f(b)


def invconv_weight(sd, prefix):
    """InvConvNear._get_weight (Glow.py:130-135) in float64, and sum log_s."""
    f = lambda k: _f(sd[prefix + k])
    l = f("l") * f("l_mask") + f("eye")
    u = f("u") * f("l_mask").T + np.diag(f("sign_s") * np.exp(f("log_s")))
    return f("p") @ (l @ u), float(f("log_s").sum())


def invconv_rows(x, w):
    """InvConvNear.forward on rows [R, 160] (Glow.py:102-127): group g mixes the channels 2g, 2g+1, 80+2g, 80+2g+1 (slots 0 .. 3)."""
    R = x.shape[0]
    v = x.reshape(R, 2, 40, 2).transpose(0, 1, 3, 2).reshape(R, 4, 40)  # [row, slot = 2a + r, group]
    z = np.einsum("on,rng->rog", _f(w), v)
    return z.reshape(R, 2, 2, 40).transpose(0, 1, 3, 2).reshape(R, 160)


def rows_forward(x, ml=None, w=None, an_bias=None, an_logs=None):
    """tts_glow_forward_rows: (x after the step, the rows' sum of logs or None).  First half: x1 = m + exp(logs) x1; second half:
    ActNorm then InvConvNear."""
    x = _f(x).copy()
    ld = None
    if ml is not None:
        ml = _f(ml)
        x[:, 80:] = ml[:, :80] + np.exp(ml[:, 80:]) * x[:, 80:]
        ld = ml[:, 80:].sum(axis=1)
    if w is not None:
        x = invconv_rows(_f(an_bias) + np.exp(_f(an_logs)) * x, w)
    return x, ld


def wavenet(h, cond, sd, p):
    """WN.forward (wavenet.py:102-119) on h [R, 192] with the conditioning cond [R, 1536] already projected -> the skip sum."""
    out = np.zeros_like(h)
    for i in range(4):
        a = conv1d(h, sd[p + f"in_layers.{i}.weight"], sd[p + f"in_layers.{i}.bias"]) + cond[:, i * 384:(i + 1) * 384]
        acts = np.tanh(a[:, :192]) / (1.0 + np.exp(-a[:, 192:]))
        rs = conv1d(acts, sd[p + f"res_skip_layers.{i}.weight"], sd[p + f"res_skip_layers.{i}.bias"])
        if i < 3:
            h = h + rs[:, :192]
            out = out + rs[:, 192:]
        else:
            out = out + rs
    return out


def logdet_constant(sd):
    """(sum over the blocks of sum an_logs, of 40 sum log_s): the parts of a row's log-determinant that no input changes."""
    an = sum(float(_f(sd[f"{FLOW}{3 * b}.logs"]).sum()) for b in range(N_BLOCKS))
    inv = sum(40.0 * invconv_weight(sd, f"{FLOW}{3 * b + 1}.")[1] for b in range(N_BLOCKS))
    return an, inv


def flow_forward(sd, gold, cat):
    """gold [T, 80]; cat [T, 272] = [refined mel | up-sampled text] (the input of g_proj) -> (z [T // 2, 160], the rows' coupling
    log-determinants [T // 2])."""
    g = squeeze(conv1d(cat, sd["post_flow.g_proj.weight"], sd["post_flow.g_proj.bias"]))
    x = squeeze(gold)
    ld = np.zeros(x.shape[0])
    for b in range(N_BLOCKS):
        pa, pn, pc = (f"{FLOW}{3 * b + i}." for i in range(3))
        x, _ = rows_forward(x, None, invconv_weight(sd, pn)[0], _f(sd[pa + "bias"]).reshape(-1), _f(sd[pa + "logs"]).reshape(-1))
        h = conv1d(x[:, :80], sd[pc + "start.weight"], sd[pc + "start.bias"])
        cond = conv1d(g, sd[pc + "wn.cond_layer.weight"], sd[pc + "wn.cond_layer.bias"])
        ml = conv1d(wavenet(h, cond, sd, pc + "wn."), sd[pc + "end.weight"], sd[pc + "end.bias"])
        x, d = rows_forward(x, ml)
        ld += d
    return x, ld


def row_parts(z, row_logdet, const):
    """[R, 2]: (sum_160 (z^2 / 2 + log(2 pi) / 2), the row's whole log-determinant = coupling part + const)."""
    z = _f(z)
    return np.stack([(0.5 * z * z + HALF_LOG_2PI).sum(axis=1), _f(row_logdet) + const], axis=1)


def loss_from_parts(parts, T):
    """Glow.py:354-356 at batch 1: the prior's mean over the truncated z, the log-determinant over the unsqueezed length T."""
    parts = _f(parts)
    rs = parts.shape[0]
    if rs == 0:
        return float("nan")
    return float(parts[:, 0].sum() / (160.0 * rs) - parts[:, 1].sum() / (80.0 * T))


def glow_loss(sd, gold, cat):
    z, ld = flow_forward(sd, gold, cat)
    return loss_from_parts(row_parts(z, ld, sum(logdet_constant(sd))), np.asarray(gold).shape[0])
