"""The aligner's on-line fine-tuning (InferenceInterfaces/UtteranceCloner.py:75-94) on the kernels of csrc/train.hip: five SGD steps
(lr 0.1, clip_grad_norm_ 1.0) of CTC training of the Aligner (AutoAligner/Aligner.py:18-75) in training mode - BatchNorm with batch
statistics and running-statistics updates, Dropout(0.5) - on the one utterance that is about to be aligned, then that utterance's
eval-mode logits from the updated parameters and running statistics.  fp32, one utterance at a time.

Every utterance starts from the checkpoint's weights (``theta0`` / ``stats0`` are never written), so a batch equals its utterances one
by one and a repeated call repeats its result.  The steps are enqueued without a host synchronisation: the clip coefficient stays on
the device; the loss and the gradient norm of every step are read back once at the end.

Layouts.  Activations are time-major [T, C]; each conv's input lives in a buffer with one zero row before and after the utterance, so
the k 3 conv is one NT product over rows that overlap (lda = Cin, K = 3 Cin), its weight gradient one TN product and its data gradient
three accumulating NN products.  Parameters and gradients are two arenas with the same offsets: conv weights as [Cout][3][Cin], the
BatchNorm weights and biases, the LSTM's weight_ih / weight_hh / bias_ih / bias_hh as torch stores them (both directions stacked),
proj.weight, proj.bias.

Dropout masks.  ``dropout_masks(seed, T)`` draws them as the reference does on a CPU device: Dropout's bernoulli_(0.5) on the
[1, T, 512] transposed view of [1, 512, T] memory, layer 1 .. 5 within a step, then the steps in order, from torch.Generator(seed).
That reproduces the reference on a CPU device bit for bit; on a GPU the reference draws from another generator that nobody can
reproduce.
"""
import numpy as np
import torch

from . import capi, engine
from .capi import GEMM_NN, GEMM_NT, GEMM_TN

N_SYMBOLS, BLANK, BN_EPS, BN_MOMENTUM = 145, 144, 1e-5, 0.1
STEPS, LAYERS, LR, MAX_NORM = 5, 5, 0.1, 1.0
N_MELS, CONV, HIDDEN = 80, 512, 512


def dropout_masks(seed, T, steps=STEPS):
    """[steps][5] boolean [T, 512] keep-masks from torch.Generator(seed), drawn as the reference's nn.Dropout(0.5) draws them on a
    CPU device."""
    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(seed))
    out = []
    for _ in range(steps):
        out.append([torch.empty(1, CONV, T).transpose(1, 2).bernoulli_(0.5, generator=gen)[0].numpy() != 0 for _ in range(LAYERS)])
    return out


def _layout():
    """name -> (offset, shape) in the parameter / gradient arena, and its size in floats."""
    H, entries, off = HIDDEN, {}, 0
    shapes = []
    for i in range(LAYERS):
        shapes.append((f"conv{i}", (CONV, 3, N_MELS if i == 0 else CONV)))
    for i in range(LAYERS):
        shapes += [(f"bn_g{i}", (CONV,)), (f"bn_b{i}", (CONV,))]
    shapes += [("w_ih", (2, 4 * H, CONV)), ("w_hh", (2, 4 * H, H)), ("b_ih", (2, 4 * H)), ("b_hh", (2, 4 * H)),
               ("proj_w", (N_SYMBOLS, 2 * H)), ("proj_b", (N_SYMBOLS,))]
    for name, shape in shapes:
        entries[name] = (off, shape)
        off += int(np.prod(shape))
    return entries, off


LAYOUT, N_PARAMS = _layout()


def pack_parameters(state_dict):
    """Reference-schema Aligner state dict -> (parameter arena [N_PARAMS] fp32, running statistics [2, 5, 512] fp32: means, variances)."""
    sd = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in state_dict.items()}
    theta = np.zeros(N_PARAMS, dtype=np.float32)

    def put(name, a):
        off, shape = LAYOUT[name]
        theta[off:off + int(np.prod(shape))] = np.asarray(a, dtype=np.float32).reshape(shape).reshape(-1)

    stats = np.zeros((2, LAYERS, CONV), dtype=np.float32)
    for i in range(LAYERS):
        c = f"convs.{2 * i}."
        put(f"conv{i}", sd[c + "conv.weight"].transpose(0, 2, 1))  # [Cout, Cin, 3] -> [Cout][3][Cin]
        put(f"bn_g{i}", sd[c + "bnorm.weight"])
        put(f"bn_b{i}", sd[c + "bnorm.bias"])
        stats[0, i], stats[1, i] = sd[c + "bnorm.running_mean"], sd[c + "bnorm.running_var"]
    for name, key in (("w_ih", "weight_ih"), ("w_hh", "weight_hh"), ("b_ih", "bias_ih"), ("b_hh", "bias_hh")):
        put(name, np.stack([sd[f"rnn.{key}_l0"], sd[f"rnn.{key}_l0_reverse"]]))
    put("proj_w", sd["proj.weight"])
    put("proj_b", sd["proj.bias"])
    return theta, stats


def unpack_parameters(theta, stats):
    """The inverse of pack_parameters (tests): arena + running statistics -> reference-schema state dict of numpy arrays."""
    theta, stats = np.asarray(theta), np.asarray(stats)
    get = lambda name: theta[LAYOUT[name][0]:LAYOUT[name][0] + int(np.prod(LAYOUT[name][1]))].reshape(LAYOUT[name][1])
    sd = {}
    for i in range(LAYERS):
        c = f"convs.{2 * i}."
        sd[c + "conv.weight"] = np.ascontiguousarray(get(f"conv{i}").transpose(0, 2, 1))
        sd[c + "bnorm.weight"], sd[c + "bnorm.bias"] = get(f"bn_g{i}").copy(), get(f"bn_b{i}").copy()
        sd[c + "bnorm.running_mean"], sd[c + "bnorm.running_var"] = stats[0, i].copy(), stats[1, i].copy()
    for name, key in (("w_ih", "weight_ih"), ("w_hh", "weight_hh"), ("b_ih", "bias_ih"), ("b_hh", "bias_hh")):
        sd[f"rnn.{key}_l0"], sd[f"rnn.{key}_l0_reverse"] = get(name)[0].copy(), get(name)[1].copy()
    sd["proj.weight"], sd["proj.bias"] = get("proj_w").copy(), get("proj_b").copy()
    return sd


def check_frames(T, what="the utterance"):
    """Torch's training-mode BatchNorm refuses one value per channel: fewer than 2 mel frames cannot be fine-tuned on."""
    if T < 2:
        raise ValueError(f"{what}: its speech span gives fewer than 2 mel frames ({T}), too few to fine-tune the aligner on")


class AlignerFineTuner:
    """Fine-tunes a copy of the aligner on one utterance and returns its eval-mode logits.  ``timing=True`` records HIP events
    around the phases (forward / ctc / bptt / gemm gradients / update / eval logits) into ``self.last_phase_ms``
    (tools/bench_finetune.py)."""

    def __init__(self, state_dict, device, timing=False, lib=None):
        self.ops = engine.Ops(device, lib=lib)
        self.device = dev = self.ops.device
        theta, stats = pack_parameters(state_dict)
        self.theta0 = torch.from_numpy(theta).to(dev)  # the checkpoint's values: never written
        self.stats0 = torch.from_numpy(stats).to(dev)
        self.theta = torch.empty_like(self.theta0)
        self.grad = torch.empty_like(self.theta0)
        self.stats = torch.empty_like(self.stats0)
        self.partials = torch.empty(capi.SUMSQ_PARTIALS, dtype=torch.float64, device=dev)
        self.timing = timing
        self.last_phase_ms = {}
        self._events = []
        self._buf_key, self._buf = None, None

    # ---- helpers --------------------------------------------------------------------------------------------------------------
    def _p(self, name, arena=None):
        off, shape = LAYOUT[name]
        return (self.theta if arena is None else arena)[off:off + int(np.prod(shape))]

    def _g(self, name):
        return self._p(name, self.grad)

    def _mark(self, name):
        if self.timing:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self._events.append((name, ev))

    def _collect(self):
        if not self.timing or not self._events:
            return
        torch.cuda.synchronize(self.device)
        ms = {}
        for (name, e0), (_, e1) in zip(self._events[:-1], self._events[1:]):
            ms[name] = ms.get(name, 0.0) + e0.elapsed_time(e1)
        self.last_phase_ms = ms
        self._events = []

    def gemm(self, op, a, lda, b, ldb, c, ldc, m, n, k, bias=None, accumulate=False):
        """a, b, c: tensors (or views into them) whose first element is the operand's."""
        capi.check(self.ops.lib.tts_gemm_f32(op, a.data_ptr(), lda, b.data_ptr(), ldb, c.data_ptr(), ldc, bias.data_ptr() if bias is not None else None,
                                             m, n, k, 1 if accumulate else 0, self.ops.stream()), "tts_gemm_f32")

    def _buffers(self, T, steps):
        """The activations, gradients and scratch of an utterance of T frames, kept for the next utterance of that length (recordings
        of one corpus are often cut to one length; the bench repeats one shape).  Every element is written before it is read in each
        call, except the zero row before and after the utterance in the padded buffers, which nothing ever writes."""
        if self._buf_key != (T, steps):
            dev, H = self.device, HIDDEN
            f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
            zp = lambda c: torch.zeros(T + 2, c, dtype=torch.float32, device=dev)
            self._buf = ([zp(c) for c in [N_MELS] + [CONV] * LAYERS],  # xpad: the conv inputs
                         [f(T, CONV) for _ in range(LAYERS)],  # z: conv outputs before the ReLU
                         f(2, LAYERS, CONV),  # batch mean, 1 / sqrt(var + eps)
                         f(T, 8 * H), f(T, 2 * H), f(T, 2, 4 * H), f(T, 2, H),  # xproj, y, gates, cseq
                         f(T, N_SYMBOLS), f(T, N_SYMBOLS), f(T, 2 * H), f(T, 8 * H), f(2, H),  # logits, dlogits, dy, dgates, dc
                         f(T, CONV), zp(CONV),  # da, dzpad
                         f(T, N_SYMBOLS), f(steps), f(steps), f(2, CONV))  # lp, loss, norm, eval scale / shift
            self._buf_key = (T, steps)
        return self._buf

    # ---- the procedure --------------------------------------------------------------------------------------------------------
    @torch.inference_mode()
    def fine_tune(self, mel, ids, masks, steps=STEPS):
        """mel: [T, 80] log-mel (tensor on any device, or array); ids: the aligner ids of the transcript's non-boundary tokens;
        masks: [steps][5] boolean [T, 512] keep-masks (``dropout_masks``).  -> eval-mode logits [T, 145] on the device after the
        steps.  Leaves ``last_loss`` / ``last_norm`` [steps] (CPU tensors) and ``theta`` / ``stats`` (the fine-tuned values)."""
        lib, dev, st, H = self.ops.lib, self.device, self.ops.stream(), HIDDEN
        mel = torch.as_tensor(mel, dtype=torch.float32)
        T, L = int(mel.shape[0]), len(ids)
        check_frames(T)
        if not 1 <= L <= capi.CTC_GRAD_MAX_TARGETS:
            raise ValueError(f"{L} tokens to align (1 .. {capi.CTC_GRAD_MAX_TARGETS})")
        m8 = np.zeros((steps, LAYERS, T, CONV), dtype=np.uint8)
        if steps:
            # (the drawn masks are transposed views: stack keeps their memory order unless told otherwise)
            m8 = np.ascontiguousarray(np.stack([np.stack([np.asarray(m, dtype=bool) for m in step]) for step in masks]), dtype=np.uint8)
        if m8.shape != (steps, LAYERS, T, CONV):
            raise ValueError(f"dropout masks of shape {m8.shape} for {steps} steps x {LAYERS} layers x [{T}, {CONV}]")
        masks_d = torch.from_numpy(m8).to(dev)
        ids_d = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).to(dev)
        self.theta.copy_(self.theta0)
        self.stats.copy_(self.stats0)
        cins = [N_MELS] + [CONV] * LAYERS
        xpad, z, save, xproj, y, gates, cseq, logits, dlogits, dy, dgates, dc, da, dzpad, lp, loss, norm, affine = self._buffers(T, steps)
        xpad[0][1:T + 1].copy_(mel.to(dev))
        alpha = torch.empty(T * (2 * L + 1), dtype=torch.float64, device=dev)
        P, G = self._p, self._g

        def conv(i):
            cin = cins[i]
            self.gemm(GEMM_NT, xpad[i], cin, P(f"conv{i}"), 3 * cin, z[i], CONV, T, CONV, 3 * cin)

        def recurrent_and_proj():
            self.gemm(GEMM_NT, xpad[LAYERS][1:], CONV, P("w_ih"), CONV, xproj, 8 * H, T, 8 * H, CONV)
            for s in range(T):
                capi.check(lib.tts_lstm_train_step(xproj.data_ptr(), 8 * H, P("w_hh").data_ptr(), P("b_ih").data_ptr(), P("b_hh").data_ptr(),
                                                   y.data_ptr(), 2 * H, gates.data_ptr(), cseq.data_ptr(), T, H, s, st), "tts_lstm_train_step")
            self.gemm(GEMM_NT, y, 2 * H, P("proj_w"), 2 * H, logits, N_SYMBOLS, T, N_SYMBOLS, 2 * H, bias=P("proj_b"))

        for step in range(steps):
            # 1. training-mode forward
            self._mark("forward")
            for i in range(LAYERS):
                conv(i)
                capi.check(lib.tts_bn_train_forward(z[i].data_ptr(), CONV, masks_d[step, i].data_ptr(), P(f"bn_g{i}").data_ptr(),
                                                    P(f"bn_b{i}").data_ptr(), self.stats[0, i].data_ptr(), self.stats[1, i].data_ptr(),
                                                    xpad[i + 1][1:].data_ptr(), CONV, save[0, i].data_ptr(), save[1, i].data_ptr(), T, CONV,
                                                    BN_EPS, BN_MOMENTUM, st), "tts_bn_train_forward")
            recurrent_and_proj()
            self._mark("ctc")
            capi.check(lib.tts_ctc_grad(logits.data_ptr(), N_SYMBOLS, N_SYMBOLS, T, ids_d.data_ptr(), L, BLANK, alpha.data_ptr(), lp.data_ptr(),
                                        loss[step:].data_ptr(), dlogits.data_ptr(), N_SYMBOLS, st), "tts_ctc_grad")
            # 2. backward: the projection, the LSTM through time, its weights, the five conv layers
            self._mark("gemm_gradients")
            self.gemm(GEMM_TN, dlogits, N_SYMBOLS, y, 2 * H, G("proj_w"), 2 * H, N_SYMBOLS, 2 * H, T)
            capi.check(lib.tts_col_sum(dlogits.data_ptr(), N_SYMBOLS, T, N_SYMBOLS, G("proj_b").data_ptr(), None, st), "tts_col_sum")
            self.gemm(GEMM_NN, dlogits, N_SYMBOLS, P("proj_w"), 2 * H, dy, 2 * H, T, 2 * H, N_SYMBOLS)
            self._mark("bptt")
            for s in range(T - 1, -1, -1):
                capi.check(lib.tts_lstm_backward_step(dy.data_ptr(), 2 * H, P("w_hh").data_ptr(), gates.data_ptr(), cseq.data_ptr(),
                                                      dgates.data_ptr(), dc.data_ptr(), T, H, s, st), "tts_lstm_backward_step")
            self._mark("gemm_gradients")
            a5 = xpad[LAYERS][1:]
            self.gemm(GEMM_TN, dgates, 8 * H, a5, CONV, G("w_ih"), CONV, 8 * H, CONV, T)
            capi.check(lib.tts_col_sum(dgates.data_ptr(), 8 * H, T, 8 * H, G("b_ih").data_ptr(), G("b_hh").data_ptr(), st), "tts_col_sum")
            # dW_hh = sum_t dgates[t] (x) h[t - 1] forwards, h[t + 1] backwards: T - 1 terms each
            ghh = G("w_hh")
            self.gemm(GEMM_TN, dgates[1:], 8 * H, y, 2 * H, ghh, H, 4 * H, H, T - 1)
            self.gemm(GEMM_TN, dgates.view(-1)[4 * H:], 8 * H, y.view(-1)[2 * H + H:], 2 * H, ghh[4 * H * H:], H, 4 * H, H, T - 1)
            self.gemm(GEMM_NN, dgates, 8 * H, P("w_ih"), CONV, da, CONV, T, CONV, 8 * H)
            for i in range(LAYERS - 1, -1, -1):
                cin = cins[i]
                capi.check(lib.tts_bn_train_backward(da.data_ptr(), CONV, z[i].data_ptr(), CONV, masks_d[step, i].data_ptr(),
                                                     P(f"bn_g{i}").data_ptr(), save[0, i].data_ptr(), save[1, i].data_ptr(), dzpad[1:].data_ptr(),
                                                     CONV, G(f"bn_g{i}").data_ptr(), G(f"bn_b{i}").data_ptr(), T, CONV, st), "tts_bn_train_backward")
                self.gemm(GEMM_TN, dzpad[1:], CONV, xpad[i], cin, G(f"conv{i}"), 3 * cin, CONV, 3 * cin, T)
                if i > 0:  # da[t] = sum_k dz[t + 1 - k] W[:, k, :]
                    for k in range(3):
                        self.gemm(GEMM_NN, dzpad[2 - k:], CONV, P(f"conv{i}")[k * cin:], 3 * cin, da, CONV, T, cin, CONV, accumulate=k > 0)
            # 3. clip and update: the norm stays on the device
            self._mark("update")
            capi.check(lib.tts_sumsq(self.grad.data_ptr(), N_PARAMS, self.partials.data_ptr(), norm[step:].data_ptr(), st), "tts_sumsq")
            capi.check(lib.tts_sgd_clip_update(self.theta.data_ptr(), self.grad.data_ptr(), N_PARAMS, norm[step:].data_ptr(), MAX_NORM, LR, st),
                       "tts_sgd_clip_update")
        # eval-mode logits from the updated parameters and running statistics
        self._mark("eval_logits")
        for i in range(LAYERS):
            conv(i)
            capi.check(lib.tts_bn_eval_affine(P(f"bn_g{i}").data_ptr(), P(f"bn_b{i}").data_ptr(), self.stats[0, i].data_ptr(),
                                              self.stats[1, i].data_ptr(), affine[0].data_ptr(), affine[1].data_ptr(), CONV, BN_EPS, st),
                       "tts_bn_eval_affine")
            capi.check(lib.tts_relu_affine(z[i].data_ptr(), CONV, xpad[i + 1][1:].data_ptr(), CONV, T, CONV, affine[0].data_ptr(),
                                           affine[1].data_ptr(), st), "tts_relu_affine")
        recurrent_and_proj()
        self._mark("end")
        self._collect()
        host = torch.stack([loss, norm]).cpu()  # the one read-back
        self.last_loss, self.last_norm = host[0], host[1]
        return logits.clone()  # (the buffer is reused by the next call)
