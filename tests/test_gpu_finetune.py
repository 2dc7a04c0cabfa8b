"""The kernels of the aligner's on-line fine-tuning (csrc/train.hip) each against a float64 yardstick, and the whole procedure
(finetune.py, align.ProsodyExtractor, UtteranceCloner(fine_tune_aligner=True)) against the reference goldens.

Tolerances.  The GEMM's is derived: an fp32 fma chain of K terms is within K * 2^-24 * sum |a_k b_k| of the exact sum.  Every other
kernel's is measured, not guessed: the same float64 yardstick (tests/finetune_ref.py) run in float32 on the CPU differs from float64
by MEASURED[...] (largest error over the largest |value| of the quantity, for BatchNorm per group of like-scaled channels); a different but equally valid fp32 order differs by about
as much, and 8 x that covers a single-sample estimate.  ``python -m tests.test_gpu_finetune`` (no GPU needed) measures and prints the
table again from the inputs below.  A quantity that is exactly zero in float64 (the zero_infinity gradient) must be exactly zero.
"""
import os

import numpy as np
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import capi, finetune, fixture_weights as fw, phonemes
from tests import aligner_ref as ar
from tests import finetune_emulator
from tests import finetune_ref as fr
from tests.finetune_cases import G, N, case, check_against_golden

DEV = "cuda:0"
H = 512

# float32-vs-float64 distance of the yardstick on the inputs below: test -> quantity -> largest error / largest |value|
MEASURED = {
    "bn_T61": {"y": 4.3e-06, "mean": 1.5e-07, "istd": 8.2e-08, "rm": 5.1e-08, "rv": 4.4e-08, "dz": 1.7e-06, "dgamma": 9.2e-06, "dbeta": 1.7e-07},
    "bn_T2": {"y": 4.6e-05, "mean": 4.7e-08, "istd": 6.6e-08, "rm": 4.6e-08, "rv": 4.0e-08, "dz": 1.0e-04, "dgamma": 2.8e-05, "dbeta": 5.3e-08},
    "lstm_T61": {"y": 8.0e-07, "dgates": 4.2e-07, "dx": 7.2e-07, "dw_ih": 5.0e-07, "dw_hh": 6.2e-07, "db_ih": 3.1e-07, "db_hh": 3.1e-07},
    "lstm_T1": {"y": 8.0e-07, "dgates": 1.7e-07, "dx": 6.2e-07, "dw_ih": 3.4e-07, "dw_hh": 0.0e+00, "db_ih": 3.5e-07, "db_hh": 3.5e-07},
    "ctc_T61_L9": {"loss": 2.6e-07, "grad": 9.0e-05},
    "ctc_repeated": {"loss": 7.6e-08, "grad": 3.1e-05},
    "ctc_exactly_feasible": {"loss": 7.2e-08, "grad": 4.8e-06},
    "ctc_infeasible": {"loss": 0.0e+00, "grad": 0.0e+00},
    "ctc_L1": {"loss": 6.8e-08, "grad": 9.2e-06},
    "ctc_S261": {"loss": 4.3e-08, "grad": 2.5e-04},
    "ctc_cap": {"loss": 8.6e-08, "grad": 3.0e-03},
    "clip_3.0": {"norms": 1.5e-08, "theta": 3.4e-08},
    "clip_0.5": {"norms": 1.3e-08, "theta": 4.5e-08},
}


# ---- inputs (seeded; shared by the tests and the measurement) -----------------------------------------------------------------
def bn_inputs(T):
    """[T, 512] pre-ReLU activations: standard normal channels; channels 64 .. 127 with mean >> deviation (5 +- 0.05); channel 7
    entirely <= 0 (its ReLU is constant 0: variance 0, istd = 1 / sqrt(eps))."""
    rng = np.random.default_rng(100 + T)
    z = rng.standard_normal((T, 512)).astype(np.float32)
    z[:, 64:128] = (5.0 + 0.05 * rng.standard_normal((T, 64))).astype(np.float32)
    z[:, 7] = -np.abs(z[:, 7])
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return {"z": z, "gamma": 1.0 + 0.2 * f(512), "beta": 0.3 * f(512), "mask": rng.random((T, 512)) < 0.5, "rm": f(512),
            "rv": (0.5 + rng.random(512)).astype(np.float32), "dy": f(T, 512)}


def lstm_inputs(T):
    rng = np.random.default_rng(200 + T)
    sd = fw.aligner_state_dict()
    w = [np.stack([np.asarray(sd[f"rnn.{k}_l0"]), np.asarray(sd[f"rnn.{k}_l0_reverse"])]).astype(np.float32)
         for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    return {"x": rng.standard_normal((T, 512)).astype(np.float32), "w": w, "dy": (0.1 * rng.standard_normal((T, 2 * H))).astype(np.float32)}


CTC_CASES = {  # name -> (frames, target ids)
    "T61_L9": (61, [3, 17, 17, 40, 5, 99, 143, 0, 21]),
    "repeated": (30, [5, 5, 7, 7, 7, 3, 3]),
    "exactly_feasible": (5, [9, 9, 12, 30]),  # 4 labels + 1 blank between the repeated pair = 5 frames: one path
    "infeasible": (3, [1, 2, 3, 4, 5, 6]),
    "L1": (10, [77]),
    "S261": (140, list((np.arange(130) * 37) % 144)),  # 261 extended states: beyond one sweep of the 256 threads
    "cap": (800, list((np.arange(768) * 37) % 144)),  # TTS_CTC_GRAD_MAX_TARGETS: 1537 states, the kernel's largest LDS layout
}


def ctc_logits(name):
    T = CTC_CASES[name][0]
    return (2.0 * np.random.default_rng(300 + T).standard_normal((T, 145))).astype(np.float32)


def clip_inputs(norm):
    rng = np.random.default_rng(400)
    g = rng.standard_normal(100003)
    return rng.standard_normal(100003).astype(np.float32), (g * (norm / np.linalg.norm(g))).astype(np.float32)


BN_GROUPS = [np.setdiff1d(np.arange(512), np.r_[7, 64:128]), np.arange(64, 128), np.array([7])]  # ordinary / shifted / constant channels


def rel(a, ref, groups=None):
    """Largest error over the largest |reference value|; an all-zero reference demands exact zeros.  groups: index sets along the
    last axis that are normalised each by their own largest value, the worst of them returned (the BatchNorm inputs hold channels of
    very different scale: 1 / sigma is 316 in the constant channel, 20 in the shifted ones and about 1.5 elsewhere)."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if groups is not None:
        return max(rel(a[..., g], ref[..., g]) for g in groups)
    top = float(np.abs(ref).max())
    err = float(np.abs(a - ref).max())
    return err / top if top > 0 else (0.0 if err == 0 else np.inf)


def groups_of(name):
    return BN_GROUPS if name.startswith("bn_") else None


def bn_yardstick(T, dtype):
    i = bn_inputs(T)
    return fr.bn_train(i["z"], i["gamma"], i["beta"], i["mask"], i["rm"], i["rv"], i["dy"], dtype=dtype)


def lstm_yardstick(T, dtype):
    i = lstm_inputs(T)
    r = fr.lstm_bptt(i["x"], *i["w"], i["dy"], dtype=dtype)
    return {k: r[k] for k in ("y", "dgates", "dx", "dw_ih", "dw_hh", "db_ih", "db_hh")}


def ctc_yardstick(name, dtype):
    loss, grad = fr.ctc_grad(ctc_logits(name), CTC_CASES[name][1], dtype=dtype)
    return {"loss": np.array([loss]), "grad": grad}


def clip_slices(g):
    """The whole gradient set and 16 odd-sized slices of it: 17 norms, so that the measured distance is the largest of 17 roundings
    and not one rounding's luck (a single fp32 norm can land on its float64 value by chance)."""
    return [g] + [g[6000 * i:6000 * i + 6007 + i] for i in range(16)]


def clip_yardstick(norm, dtype):
    p, g = clip_inputs(norm)
    return {"norms": np.array([fr.clip_update(p[:len(s)], s, dtype=dtype)[0] for s in clip_slices(g)]), "theta": fr.clip_update(p, g, dtype=dtype)[1]}


YARDSTICKS = [(f"bn_T{T}", bn_yardstick, T) for T in (61, 2)] + [(f"lstm_T{T}", lstm_yardstick, T) for T in (61, 1)] + \
             [(f"ctc_{n}", ctc_yardstick, n) for n in CTC_CASES] + [(f"clip_{n}", clip_yardstick, n) for n in (3.0, 0.5)]
_REF = {}


def yardstick(name):
    if name not in _REF:
        fn, arg = {n: (f, a) for n, f, a in YARDSTICKS}[name]
        _REF[name] = fn(arg, torch.float64)
    return _REF[name]


def check(name, got):
    ref, errs = yardstick(name), {}
    for k, v in got.items():
        errs[k] = (rel(v, ref[k], groups_of(name)), 8.0 * MEASURED[name][k])
    print(f"{name}: " + ", ".join(f"{k} {e:.1e} (bound {b:.1e})" for k, (e, b) in errs.items()))
    assert all(e <= b for e, b in errs.values()), {k: v for k, v in errs.items() if v[0] > v[1]}


def measure():
    for name, fn, arg in YARDSTICKS:
        a, b = fn(arg, torch.float32), fn(arg, torch.float64)
        print(f'    "{name}": {{' + ", ".join(f'"{k}": {rel(a[k], b[k], groups_of(name)):.1e}' for k in b) + "},")


# ---- device helpers -----------------------------------------------------------------------------------------------------------
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return capi.lib()


def dv(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def zeros(*shape):
    return torch.zeros(*shape, dtype=torch.float32, device=DEV)


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def gemm(lib, op, a, lda, b, ldb, c, ldc, m, n, k, bias=None, accumulate=False):
    capi.check(lib.tts_gemm_f32(op, a.data_ptr(), lda, b.data_ptr(), ldb, c.data_ptr(), ldc, bias.data_ptr() if bias is not None else None, m, n, k,
                                int(accumulate), stream()), "tts_gemm_f32")


# ---- GEMM ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [capi.GEMM_NN, capi.GEMM_NT, capi.GEMM_TN])
@pytest.mark.parametrize("m,n,k", [(97, 145, 240), (512, 1536, 61), (61, 512, 1536)])
def test_gemm_f32(lib, op, m, n, k):
    """Every element within K * 2^-24 * sum_k |a_k b_k| of the float64 product (the fp32 accumulation bound; the accumulate form
    and the bias add two more roundings of a sum that also holds |c| and |bias|: (K + 2) * 2^-24 * (sum |a b| + |c| + |bias|)).
    Leading dimensions larger than the widths; the elements between the rows and around C must stay untouched."""
    rng = np.random.default_rng(m + n + k + op)
    A, B = rng.standard_normal((m, k)).astype(np.float32), rng.standard_normal((k, n)).astype(np.float32)
    sa, sb = (A.T if op == capi.GEMM_TN else A), (B.T if op == capi.GEMM_NT else B)
    lda, ldb, ldc = sa.shape[1] + 3, sb.shape[1] + 5, n + 7
    ad, bd = zeros(sa.shape[0], lda), zeros(sb.shape[0], ldb)
    ad[:, :sa.shape[1]] = dv(sa)
    bd[:, :sb.shape[1]] = dv(sb)
    exact = A.astype(np.float64) @ B.astype(np.float64)
    mag = np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64)
    cd = torch.full((m + 1, ldc), 7.0, dtype=torch.float32, device=DEV)
    gemm(lib, op, ad, lda, bd, ldb, cd, ldc, m, n, k)
    got = cd.cpu().numpy().astype(np.float64)
    worst = float((np.abs(got[:m, :n] - exact) / (k * 2.0 ** -24 * mag)).max())
    print(f"gemm op {op} {m} x {n} x {k}: largest error {worst:.3f} of the bound")
    assert worst <= 1.0
    assert (got[:m, n:] == 7.0).all() and (got[m] == 7.0).all()
    # accumulate + bias
    c0, bias = rng.standard_normal((m, n)).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    cd[:m, :n] = dv(c0)
    gemm(lib, op, ad, lda, bd, ldb, cd, ldc, m, n, k, bias=dv(bias), accumulate=True)
    got = cd.cpu().numpy().astype(np.float64)
    bound = (k + 2) * 2.0 ** -24 * (mag + np.abs(c0) + np.abs(bias)[None])
    assert float((np.abs(got[:m, :n] - (exact + c0 + bias[None])) / bound).max()) <= 1.0
    assert (got[:m, n:] == 7.0).all() and (got[m] == 7.0).all()


def test_gemm_f32_odd_and_empty_k(lib):
    """K = 1, an odd K below one MFMA step pair, and K = 0 (the T = 1 recurrent weight gradient): zeros, or the bias."""
    rng = np.random.default_rng(9)
    for k in (1, 3):
        A, B = rng.standard_normal((5, k)).astype(np.float32), rng.standard_normal((k, 70)).astype(np.float32)
        cd = zeros(5, 70)
        gemm(lib, capi.GEMM_NN, dv(A), k, dv(B), 70, cd, 70, 5, 70, k)
        exact, mag = A.astype(np.float64) @ B, np.abs(A).astype(np.float64) @ np.abs(B)
        assert float((np.abs(cd.cpu().numpy() - exact) / (k * 2.0 ** -24 * mag)).max()) <= 1.0
    cd = torch.full((5, 70), 3.0, dtype=torch.float32, device=DEV)
    bias = dv(rng.standard_normal(70).astype(np.float32))
    gemm(lib, capi.GEMM_TN, cd, 5, cd, 70, cd, 70, 5, 70, 0)
    assert not cd.any()
    gemm(lib, capi.GEMM_TN, cd, 5, cd, 70, cd, 70, 5, 70, 0, bias=bias)
    assert torch.equal(cd, bias[None].expand(5, 70))


# ---- BatchNorm ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [61, 2])
def test_bn_train_forward_and_backward(lib, T):
    i, C = bn_inputs(T), 512
    z, mask, gamma, beta, rm, rv, dy = dv(i["z"]), dv(i["mask"].astype(np.uint8), torch.uint8), dv(i["gamma"]), dv(i["beta"]), dv(i["rm"]), \
        dv(i["rv"]), dv(i["dy"])
    y, mean, istd, dz, dg, db = zeros(T, C), zeros(C), zeros(C), zeros(T, C), zeros(C), zeros(C)
    capi.check(lib.tts_bn_train_forward(z.data_ptr(), C, mask.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(),
                                        y.data_ptr(), C, mean.data_ptr(), istd.data_ptr(), T, C, 1e-5, 0.1, stream()), "tts_bn_train_forward")
    capi.check(lib.tts_bn_train_backward(dy.data_ptr(), C, z.data_ptr(), C, mask.data_ptr(), gamma.data_ptr(), mean.data_ptr(), istd.data_ptr(),
                                         dz.data_ptr(), C, dg.data_ptr(), db.data_ptr(), T, C, stream()), "tts_bn_train_backward")
    got = {k: v.cpu().numpy() for k, v in (("y", y), ("mean", mean), ("istd", istd), ("rm", rm), ("rv", rv), ("dz", dz), ("dgamma", dg), ("dbeta", db))}
    check(f"bn_T{T}", got)
    assert got["mean"][7] == 0.0 and abs(got["istd"][7] - 1.0 / np.sqrt(1e-5)) <= 1e-4 and not got["dz"][:, 7].any()  # the constant channel
    assert (got["y"][~i["mask"]] == 0).all()


# ---- LSTM ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [61, 1])
def test_lstm_train_and_backward_steps(lib, T):
    """Forward: y against aligner_ref.lstm_reference on the device's own input projection.  BPTT, and the products and column sums
    that finetune.py forms from its gate gradients, against float64 autograd of torch.nn.LSTM(512, 512, bidirectional=True)."""
    i = lstm_inputs(T)
    x, dy = dv(i["x"]), dv(i["dy"])
    w_ih, w_hh, b_ih, b_hh = (dv(a) for a in i["w"])
    xproj, y, gates, cseq, dgates, dc = zeros(T, 8 * H), zeros(T, 2 * H), zeros(T, 2, 4 * H), zeros(T, 2, H), zeros(T, 8 * H), zeros(2, H)
    gemm(lib, capi.GEMM_NT, x, 512, w_ih, 512, xproj, 8 * H, T, 8 * H, 512)
    for s in range(T):
        capi.check(lib.tts_lstm_train_step(xproj.data_ptr(), 8 * H, w_hh.data_ptr(), b_ih.data_ptr(), b_hh.data_ptr(), y.data_ptr(), 2 * H,
                                           gates.data_ptr(), cseq.data_ptr(), T, H, s, stream()), "tts_lstm_train_step")
    for s in range(T - 1, -1, -1):
        capi.check(lib.tts_lstm_backward_step(dy.data_ptr(), 2 * H, w_hh.data_ptr(), gates.data_ptr(), cseq.data_ptr(), dgates.data_ptr(),
                                              dc.data_ptr(), T, H, s, stream()), "tts_lstm_backward_step")
    dx, dw_ih, dw_hh, db1, db2 = zeros(T, 512), zeros(2, 4 * H, 512), torch.full((2, 4 * H, H), 9.0, dtype=torch.float32, device=DEV), \
        zeros(2, 4 * H), zeros(2, 4 * H)
    gemm(lib, capi.GEMM_NN, dgates, 8 * H, w_ih, 512, dx, 512, T, 512, 8 * H)
    gemm(lib, capi.GEMM_TN, dgates, 8 * H, x, 512, dw_ih, 512, 8 * H, 512, T)
    gemm(lib, capi.GEMM_TN, dgates[1:], 8 * H, y, 2 * H, dw_hh, H, 4 * H, H, T - 1)
    gemm(lib, capi.GEMM_TN, dgates.view(-1)[4 * H:], 8 * H, y.view(-1)[3 * H:], 2 * H, dw_hh[1], H, 4 * H, H, T - 1)
    capi.check(lib.tts_col_sum(dgates.data_ptr(), 8 * H, T, 8 * H, db1.data_ptr(), db2.data_ptr(), stream()), "tts_col_sum")
    # forward against the float64 recurrence on the device's input projection
    bias = (i["w"][2].astype(np.float64) + i["w"][3]).reshape(-1)
    want = ar.lstm_reference(xproj.cpu().numpy().astype(np.float64) + bias[None], i["w"][1].transpose(0, 2, 1), [T], H)
    assert float(np.abs(y.cpu().numpy() - want).max()) <= 8.0 * MEASURED[f"lstm_T{T}"]["y"] * float(np.abs(want).max())
    c = cseq.cpu().numpy()
    assert np.allclose(y.cpu().numpy().reshape(T, 2, H), gates.cpu().numpy()[:, :, 3 * H:] * np.tanh(c), rtol=0, atol=1e-6)
    check(f"lstm_T{T}", {"y": y.cpu().numpy(), "dgates": dgates.cpu().numpy(), "dx": dx.cpu().numpy(), "dw_ih": dw_ih.cpu().numpy(),
                         "dw_hh": dw_hh.cpu().numpy(), "db_ih": db1.cpu().numpy(), "db_hh": db2.cpu().numpy()})


# ---- CTC ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CTC_CASES))
def test_ctc_grad(lib, name):
    T, ids = CTC_CASES[name]
    L, ld = len(ids), 150
    lg = torch.full((T, ld), float("nan"), dtype=torch.float32, device=DEV)  # the padding columns are never read
    lg[:, :145] = dv(ctc_logits(name))
    grad = torch.full((T, ld), 5.0, dtype=torch.float32, device=DEV)
    alpha, lp, loss = torch.empty(T * (2 * L + 1), dtype=torch.float64, device=DEV), zeros(T, 145), zeros(1)
    targets = dv(np.int32(ids), torch.int32)
    capi.check(lib.tts_ctc_grad(lg.data_ptr(), ld, 145, T, targets.data_ptr(), L, 144, alpha.data_ptr(), lp.data_ptr(),
                                loss.data_ptr(), grad.data_ptr(), ld, stream()), "tts_ctc_grad")
    g = grad.cpu().numpy()
    check(f"ctc_{name}", {"loss": loss.cpu().numpy(), "grad": g[:, :145]})
    assert (g[:, 145:] == 5.0).all()
    # A tighter, derived check beside the measured one (whose float32 yardstick is torch's float32 recursion, far less exact than the
    # kernel's float64 one).  The kernel's log-probabilities: x - max is one rounding, the sum of 145 exponentials at most 145 more, the
    # logarithm and the last subtraction three: within (145 + 4) * 2^-24 (+ one spacing of the largest |lp|) of the float64 log-softmax.
    # From those very log-probabilities a float64 recursion in another order differs from the kernel's by about T * 2^-52, so what is
    # left is the rounding of the result to float32: 2^-24 of an element, allowed twice over, relative to the largest.
    x64 = ctc_logits(name).astype(np.float64)
    lp64 = x64 - x64.max(1, keepdims=True) - np.log(np.exp(x64 - x64.max(1, keepdims=True)).sum(1, keepdims=True))
    lp_h = lp.cpu().numpy()
    assert float(np.abs(lp_h - lp64).max()) <= 149 * 2.0 ** -24 + float(np.spacing(np.float32(np.abs(lp64).max())))
    loss2, grad2 = finetune_emulator.ctc_from_log_probs(lp_h, ids, 144)
    assert float(np.abs(g[:, :145] - grad2).max()) <= 2.0 ** -23 * float(np.abs(grad2).max())
    assert abs(float(loss) - loss2) <= 2.0 ** -23 * loss2
    if name == "infeasible":
        assert float(loss) == 0.0 and not g[:, :145].any()
    else:
        assert float(loss) > 0 and np.abs(g[:, :145].sum(1)).max() < 1e-6  # softmax - posterior: every frame's row sums to 0


# ---- clip and update ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [3.0, 0.5])
def test_sumsq_and_sgd_clip_update(lib, norm):
    p, g = clip_inputs(norm)
    pd, gd, nd = dv(p), dv(g), zeros(1)
    partials = torch.empty(capi.SUMSQ_PARTIALS, dtype=torch.float64, device=DEV)
    norms = zeros(17)
    for k, sl in enumerate(clip_slices(gd)):
        capi.check(lib.tts_sumsq(sl.data_ptr(), sl.numel(), partials.data_ptr(), norms[k:].data_ptr(), stream()), "tts_sumsq")
    capi.check(lib.tts_sumsq(gd.data_ptr(), g.size, partials.data_ptr(), nd.data_ptr(), stream()), "tts_sumsq")
    capi.check(lib.tts_sgd_clip_update(pd.data_ptr(), gd.data_ptr(), g.size, nd.data_ptr(), 1.0, 0.1, stream()), "tts_sgd_clip_update")
    check(f"clip_{norm}", {"norms": norms.cpu().numpy(), "theta": pd.cpu().numpy()})
    assert float(nd) == float(norms[0])
    moved = float(np.abs(pd.cpu().numpy() - p).max() / np.abs(g).max())
    assert abs(moved - 0.1 * min(1.0, 1.0 / norm)) < 1e-4  # clipped above norm 1, plain SGD below


# ---- end to end ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tuner():
    return finetune.AlignerFineTuner(fw.aligner_state_dict(), DEV)


@pytest.mark.parametrize("c", range(N))
def test_fine_tuning_against_the_reference(tuner, c):
    """The golden cases through finetune.py with the stored masks: per-step loss and norm, running statistics and fine-tuned logits
    within 8 x the reference's own fp32-vs-fp64 distance (floor 1e-5 of the largest |logit|), durations exact; a repeated call
    repeats every bit, and the checkpoint's copy of the weights stays as loaded."""
    mel, ids, masks = case(c)
    logits = tuner.fine_tune(mel, ids, masks).clone()
    check_against_golden(c, logits.cpu().numpy(), tuner.last_loss.numpy(), tuner.last_norm.numpy(), tuner.stats[0].cpu().numpy(),
                         tuner.stats[1].cpu().numpy())
    theta = tuner.theta.clone()
    assert torch.equal(tuner.fine_tune(mel, ids, masks), logits) and torch.equal(tuner.theta, theta)
    theta0, stats0 = finetune.pack_parameters(fw.aligner_state_dict())
    assert np.array_equal(tuner.theta0.cpu().numpy(), theta0) and np.array_equal(tuner.stats0.cpu().numpy(), stats0)
    assert float((theta - tuner.theta0).norm()) > 0.1  # (0.23 - 0.24 on these inputs: every step is clipped to a move of 0.1)


def test_extraction_with_fine_tuning_against_the_reference():
    """align.ProsodyExtractor with fine_tune=: the golden mels in one ragged batch with the stored masks -> the reference's durations
    (word boundaries and repeated phonemes included) exactly; the batch equals each utterance alone bit for bit; the result differs
    from the eval-mode one."""
    from ims_toucan_prosody_variance_amd import align
    ex = align.ProsodyExtractor(fw.aligner_state_dict(), DEV)
    feats = [phonemes.phones_to_features(str(G[f"ft{c}_phones"]), handle_missing=False) for c in range(N)]
    mels = [case(c)[0] for c in range(N)]
    masks = [case(c)[2] for c in range(N)]
    waves = [fw.reference_wave(500 + c, 256 * (len(m) - 1) + 9) for c, m in enumerate(mels)]
    res = ex.extract(feats, waves, mels=mels, fine_tune=masks)
    lg, rag = ex.last_logits.clone(), ex.last_rag
    for c in range(N):
        assert np.array_equal(res[c][0].numpy(), G[f"ft{c}_dur"]), c
        one = ex.extract([feats[c]], [waves[c]], mels=[mels[c]], fine_tune=[masks[c]])[0]
        assert torch.equal(one[0], res[c][0]) and torch.equal(one[2], res[c][2])
        assert torch.equal(ex.last_logits[:rag.lengths[c]], lg[rag.begins[c]:rag.begins[c] + rag.lengths[c]]), c
    ex.extract(feats, waves, mels=mels)
    rows = torch.cat([torch.arange(b0, b0 + n) for b0, n in zip(rag.begins, rag.lengths)]).to(DEV)  # (the rows between utterances hold nothing)
    moved = float((ex.last_logits[rows] - lg[rows]).abs().max())
    print(f"fine-tuning moves the logits by {moved:.2f} (largest |logit| before {float(ex.last_logits[rows].abs().max()):.2f})")
    assert moved > 1.0  # 2.6 - 2.8 on these inputs (printed by the golden maker), five orders of magnitude above the comparison tolerance


# The cloner's recording: fixture_weights.reference_wave(CLONER_SEED, CLONER_SAMPLES), 61 frames, with the dropout masks of the same
# seed.  Chosen like the goldens' inputs, by the yardstick on the CPU (float64 restatement of the log-mel of this recording): seeds 20 .. 43
# give fp32-vs-fp64 distances of the fine-tuned logits from 1.7e-6 to 3.3e-2 of the largest |logit|; this one gives 2.5e-5 (CLONER_SENS),
# with the per-step losses 9.0e-7 and norms 2.6e-5 apart and a MAS margin of 44 072 ulps.
CLONER_PHONES, CLONER_SEED, CLONER_SAMPLES, CLONER_SENS = "~həlˈoʊ wˈɜːld~#", 36, 256 * 60 + 77, 2.5e-5


def test_utterance_cloner_with_fine_tuning(tmp_path, monkeypatch):
    """UtteranceCloner(fine_tune_aligner=True) against what is computed outside it.  On the cloner's own log-mel of the recording
    and the seed's masks given as dropout_masks=: the float64 yardstick (finetune_ref) - fine-tuned logits, per-step loss and norm
    within 8 x CLONER_SENS (floor 1e-5, the goldens' rule), durations equal to MAS + the duration repair on the yardstick's logits -
    and a separately built finetune.AlignerFineTuner, bit for bit.  Then the interface: no warning; the seed's own masks give the
    same; a batch equals one by one; on_line_fine_tune=False and a plain instance give the eval-mode result, which differs; the
    cloned wave is the plain synthesis with the fine-tuned prosody."""
    import warnings
    from ims_toucan_prosody_variance_amd import align, interface, style
    CLONE_G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aligner", "aligner.npz"))
    models = tmp_path / "Models"
    interface.write_fixture_checkpoints(str(models), n_lang=20)
    interface.write_fixture_aligner_checkpoint(str(models))
    monkeypatch.setattr(interface, "MODELS_DIR", str(models))
    from InferenceInterfaces.UtteranceCloner import UtteranceCloner
    phones = [CLONER_PHONES, str(CLONE_G["clone_phones"][2])]
    wavs = [fw.reference_wave(CLONER_SEED, CLONER_SAMPLES), fw.reference_wave(int(CLONE_G["clone2_seed"]), int(CLONE_G["clone2_samples"]))]
    ref_wav = str(tmp_path / "ref.wav")
    interface.write_wav(ref_wav, wavs[0], 16000)
    tuned = UtteranceCloner(model_id=str(models / "ToucanTTS_Meta" / "best.pt"), device=DEV, language="en", fine_tune_aligner=True,
                            fine_tune_seed=CLONER_SEED)
    T = 1 + CLONER_SAMPLES // 256
    masks = finetune.dropout_masks(CLONER_SEED, T)
    with warnings.catch_warnings():
        warnings.simplefilter("error", UserWarning)
        d, p, e, s0, s1 = tuned.extract_prosody(phones[0], ref_wav, lang="en", dropout_masks=masks)
    ex = tuned.extractor
    assert ex.last_rag.lengths[0] == T and p is None and s0 == 0 and s1 == 0
    ft_logits = ex.last_logits[:T].clone()
    loss, norm = (v.numpy() for v in ex.last_fine_tune[0])
    mel = ex.last_mel[:T].cpu().numpy()
    # outside the cloner: the float64 yardstick on the same log-mel and masks
    ids, flags = align.token_ids(phonemes.phones_to_features(phones[0], handle_missing=False))
    r = fr.fine_tune(fw.aligner_state_dict(), mel, ids, masks)
    bound, top = max(8.0 * CLONER_SENS, 1e-5), float(np.abs(r["logits"]).max())
    errs = {"logits": float(np.abs(ft_logits.cpu().numpy() - r["logits"]).max()) / top,
            "loss": float(np.abs(loss - r["loss"]).max() / r["loss"].max()), "norm": float(np.abs(norm - r["norm"]).max() / r["norm"].max())}
    print("cloner against the float64 yardstick: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()) + f" (bound {bound:.1e})")
    assert all(v <= bound for v in errs.values()), errs
    want_nb, _, ulps = ar.mas(r["logits"].astype(np.float32)[:, ids], log64=True)
    assert ulps >= 64 and np.array_equal(d.numpy(), ar.postprocess(want_nb, flags))
    # outside the cloner: another instance of the device path
    other = finetune.AlignerFineTuner(fw.aligner_state_dict(), DEV)
    assert torch.equal(other.fine_tune(mel, ids, masks), ft_logits)
    assert np.array_equal(other.last_loss.numpy(), loss) and np.array_equal(other.last_norm.numpy(), norm)
    # the interface
    drawn = tuned.extract_prosody(phones[0], ref_wav, lang="en")  # the masks of fine_tune_seed
    assert torch.equal(drawn[0], d) and torch.equal(drawn[2], e)
    wave0 = style.read_audio(ref_wav)[0]
    both = tuned.extract_prosody_batch(phones, [wave0, wavs[1]], 16000)
    assert torch.equal(both[0][0], d) and torch.equal(both[0][2], e)
    one = tuned.extract_prosody_batch([phones[1]], [wavs[1]], 16000)[0]
    assert torch.equal(one[0], both[1][0]) and torch.equal(one[2], both[1][2])
    off = tuned.extract_prosody(phones[0], ref_wav, lang="en", on_line_fine_tune=False)
    eval_logits = ex.last_logits[:T].clone()
    plain = UtteranceCloner(model_id=str(models / "ToucanTTS_Meta" / "best.pt"), device=DEV, language="en")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = plain.extract_prosody(phones[0], ref_wav, lang="en")
    assert torch.equal(off[0], base[0]) and torch.equal(off[2], base[2]) and torch.equal(plain.extractor.last_logits[:T], eval_logits)
    moved = float((ft_logits - eval_logits).abs().max())
    print(f"cloner: fine-tuning moves the logits by {moved:.2f}; durations {d.tolist()} (eval mode: {base[0].tolist()})")
    assert moved > 0.1  # four orders of magnitude above the 1e-5 by which two correct float32 results differ
    z = torch.from_numpy(fw.normal("clone.z", (80, int(d.sum())), 1, 0.8))
    cloned = tuned.clone_utterance(ref_wav, ref_wav, phones[0], lang="en", z_noise=z)
    want = tuned.tts(phones[0], durations=d, pitch=None, energy=e, input_is_phones=True, z_noise=z).cpu().numpy()
    assert np.array_equal(cloned, want)


if __name__ == "__main__":
    measure()
