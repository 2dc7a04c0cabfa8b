"""TEST INFRASTRUCTURE ONLY: the seeded inputs, the float64 references and the assertions shared by
tests/test_gpu_kernels_long_shapes.py (the HIP kernels on the MI355X) and tests/test_long_shape_references_cpu.py (the references
themselves, and the ABI emulator at the same shapes).  Every shape is the smallest that makes a kernel's loop turn over: a second
sweep of 256 items, a second chunk of 8 utterances, a grid past its cap.  A case is built once per process (lru_cache) and is
read-only: the runners copy what a kernel overwrites.

``run_*(ops, to, ...)`` runs one entry point through ``ops`` (engine.Ops on the GPU, or on the emulator) with tensors moved by
``to`` (see ``mover``); ``check_*`` holds the result to the float64 reference and returns the largest error it saw."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from ims_toucan_prosody_variance_amd.ragged import Ragged
from oracle import toucan_oracle as oracle
from tests import aligner_ref as ar
from tests import scorer_ref as sr

TOL32 = 2e-5  # fp32 kernels: relative to the output scale
SENTINEL = -777.0


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def as32(t):
    """float64 tensor holding the fp32 values a kernel sees."""
    return t.float().double()


def mover(device):
    """Floating tensors go to `device` as fp32, integer tensors unchanged; always a fresh contiguous copy."""
    def to(t):
        t = t.to(torch.float32) if t.is_floating_point() else t
        return t.clone().to(device).contiguous()
    return to


def host(t):
    return t.detach().cpu()


def max_err(got, want, tol, what=""):
    """`close` of test_gpu_kernels_vs_float64 with NaN support: the NaN positions must agree, the rest lies within tol of the
    output scale.  Returns the error relative to that scale."""
    got, want = host(got).double().numpy(), host(want).double().numpy()
    assert got.shape == want.shape, f"{what} shape {got.shape} vs {want.shape}"
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what} NaN at {int(np.isnan(got).sum())} places, the reference at {int(nan.sum())}"
    if nan.all():
        return 0.0
    assert np.isfinite(got[~nan]).all(), f"{what} not finite"
    scale = max(1.0, float(np.abs(want[~nan]).max()))
    err = float(np.abs(got[~nan] - want[~nan]).max())
    assert err <= tol * scale, f"{what} max abs err {err:.3e} vs tol {tol * scale:.3e}"
    return err / scale


def begins_of(lengths):
    return [int(b) for b in np.concatenate([[0], np.cumsum(lengths)[:-1]])]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. length regulator
# ---------------------------------------------------------------------------------------------------------------------------
LR_LENGTHS, LR_C, LR_DEC_SCALE = [1, 255, 256, 257, 600, 4096], 192, 13.0


def length_regulate_f64(enc, pitch, energy, wp, bp, we, be, dur):
    """One utterance: repeat_interleave(enc + (p * wp + bp) + (e * we + be), dur); all-zero durations become all ones."""
    v = enc + (pitch[:, None] * wp + bp) + (energy[:, None] * we + be)
    return oracle.length_regulate(v, dur.long())


@functools.lru_cache(maxsize=None)
def length_regulate_case():
    g = torch.Generator().manual_seed(21)
    durs = [torch.randint(0, 6, (n,), generator=g, dtype=torch.int32) for n in LR_LENGTHS]
    durs[0][:] = 3
    durs[1][:] = 0                      # L = 255 all zero: becomes all ones, beside utterances that are not
    durs[2][-7:], durs[2][-8] = 0, 2    # a run of zeros at the end, up to the edge of the first sweep
    durs[3][:10], durs[3][10] = 0, 2    # a run of zeros at the start
    durs[4][106:406], durs[4][105], durs[4][406] = 0, 1, 4  # 300 zeros straddling index 256
    durs[5][-40:], durs[5][-41] = 0, 5  # a run at the end of the last sweep
    R = sum(LR_LENGTHS)
    c = SimpleNamespace(durs=durs, dur=torch.cat(durs), enc=as32(rnd(R, LR_C, seed=1)), pitch=as32(rnd(R, seed=2)),
                        energy=as32(rnd(R, seed=3).abs()), wp=as32(rnd(LR_C, seed=6)), bp=as32(rnd(LR_C, seed=7)),
                        we=as32(rnd(LR_C, seed=8)), be=as32(rnd(LR_C, seed=9)))
    c.want = []
    for b0, n, d in zip(begins_of(LR_LENGTHS), LR_LENGTHS, durs):
        c.want.append(length_regulate_f64(c.enc[b0:b0 + n], c.pitch[b0:b0 + n], c.energy[b0:b0 + n], c.wp, c.bp, c.we, c.be, d))
    c.frames = [int(w.shape[0]) for w in c.want]
    return c


def run_length_regulate(ops, to, lengths=None):
    """-> (up, dec_in, frame layout).  Both outputs start as the sentinel, three rows longer than the layout."""
    c = length_regulate_case()
    ragp = Ragged(LR_LENGTHS if lengths is None else lengths, ops.device)
    ragf = Ragged(c.frames, ops.device, align=2)
    up = to(torch.full((ragf.total_rows + 3, LR_C), SENTINEL))
    dec = to(torch.full((ragf.total_rows + 3, LR_C), SENTINEL))
    ops.length_regulate(to(c.enc), to(c.pitch), to(c.energy), to(c.wp), to(c.bp), to(c.we), to(c.be), to(c.dur), ragp, ragf, up, dec,
                        LR_DEC_SCALE)
    return up, dec, ragf


def check_length_regulate(up, dec, ragf):
    c = length_regulate_case()
    up, dec = host(up), host(dec)
    outside = torch.ones(up.shape[0], dtype=torch.bool)
    worst = 0.0
    for b0, n, want in zip(ragf.begins, ragf.lengths, c.want):
        assert n == want.shape[0]
        outside[b0:b0 + n] = False
        worst = max(worst, max_err(up[b0:b0 + n], want, TOL32, f"up, {n} frames:"))
        worst = max(worst, max_err(dec[b0:b0 + n], want * LR_DEC_SCALE, TOL32, f"dec_in, {n} frames:"))
    assert outside.sum() >= 3 + 1  # (the three spare rows, and a gap after an odd frame count)
    assert (up[outside] == SENTINEL).all() and (dec[outside] == SENTINEL).all(), "rows outside every utterance were written"
    return worst


# ---------------------------------------------------------------------------------------------------------------------------
# 2. prosody control
# ---------------------------------------------------------------------------------------------------------------------------
PC_LENGTHS = [1000, 257, 256, 3]
PC_UNVOICED = 1  # the utterance whose pitch is entirely unvoiced
# (duration, pitch variance, energy variance, pause)
PC_SCALES = [(1.0, 1.0, 1.0, 1.0), (1.2, 1.3, 0.7, 1.2), (0.5, 2.0, 0.0, 0.5)]


@functools.lru_cache(maxsize=None)
def prosody_case():
    R = sum(PC_LENGTHS)
    g = torch.Generator().manual_seed(31)
    text = (torch.rand(R, 62, generator=g) < 0.3).float()
    begins = begins_of(PC_LENGTHS)
    for u, (b0, n) in enumerate(zip(begins, PC_LENGTHS)):
        text[b0, oracle.F_VOICED], text[b0, oracle.F_PHONEME] = 1.0, 1.0
        if u == PC_UNVOICED:
            text[b0:b0 + n, oracle.F_VOICED] = 0.0
    # multiples of 4: d * 0.5, round(d * 0.5) * 0.5 and every product with 1.2 stay clear of a half (asserted by the tests)
    dur = 4 * torch.randint(0, 6, (R,), generator=g, dtype=torch.int32)
    return SimpleNamespace(text=text, pitch=as32(rnd(R, seed=2)), energy=as32(rnd(R, seed=3).abs()), dur=dur, begins=begins)


def prosody_f64(scales):
    """Per utterance, the oracle's restatement of InferenceToucanTTS.py:214-227 and _scale_variance: float64 pitch and energy,
    torch.round (half to even) on fp32 products for the durations."""
    c = prosody_case()
    ds, ps, es, pause = scales
    p, e, d = [], [], []
    for b0, n in zip(c.begins, PC_LENGTHS):
        pu, eu, du = oracle.control(c.text[b0:b0 + n], c.pitch[b0:b0 + n], c.energy[b0:b0 + n], c.dur[b0:b0 + n].long(), ds, ps, es, pause)
        p.append(pu), e.append(eu), d.append(du)
    return torch.cat(p), torch.cat(e), torch.cat(d)


def prosody_half_distance(scales):
    """Smallest distance to k + 0.5 of any product the duration path rounds (the scale as the fp32 value the kernel multiplies by)."""
    c = prosody_case()
    ds, _, _, pause = (float(np.float32(s)) for s in scales)
    d = c.dur.double().clone()
    d[c.text[:, oracle.F_WORD_BOUNDARY] == 1] = 0.0
    worst = math.inf
    if pause != 1.0:
        sil = c.text[:, oracle.F_SILENCE] == 1
        prod = d[sil] * pause
        worst = min(worst, float(((prod - torch.floor(prod)) - 0.5).abs().min()))
        d[sil] = torch.round(prod)
    if ds != 1.0:
        prod = d * ds
        worst = min(worst, float(((prod - torch.floor(prod)) - 0.5).abs().min()))
    return worst


def run_prosody(ops, to, scales):
    c = prosody_case()
    rag = Ragged(PC_LENGTHS, ops.device)
    p, e, d = to(c.pitch), to(c.energy), to(c.dur)
    ops.prosody_control(to(c.text), p, e, d, rag, *scales)
    return p, e, d


def check_prosody(p, e, d, scales):
    c = prosody_case()
    wp, we, wd = prosody_f64(scales)
    assert torch.equal(host(d).long(), wd), "durations"
    b0, n = c.begins[PC_UNVOICED], PC_LENGTHS[PC_UNVOICED]
    assert bool(torch.isnan(wp[b0:b0 + n]).all()) == (scales[1] != 1.0) and int(torch.isnan(wp).sum()) in (0, n)
    if scales == (1.0, 1.0, 1.0, 1.0):  # nothing may change but the masking
        assert torch.equal(host(p).double(), wp) and torch.equal(host(e).double(), we)
    return max(max_err(p, wp, TOL32, "pitch:"), max_err(e, we, TOL32, "energy:"))


# ---------------------------------------------------------------------------------------------------------------------------
# 3. duration head
# ---------------------------------------------------------------------------------------------------------------------------
DUR_N, DUR_EXCUSED_MAX, DUR_HALF_REL = 4096, 80, 2e-6


@functools.lru_cache(maxsize=None)
def duration_case():
    halves = torch.log(torch.arange(64, dtype=torch.float64) + 1.5)
    x = torch.cat([torch.linspace(-5.0, 6.0, DUR_N - 67, dtype=torch.float64), torch.tensor([-100.0, 20.0, 89.0], dtype=torch.float64),
                   halves]).float()
    assert x.numel() == DUR_N
    want = torch.clamp(torch.clamp(torch.round(torch.exp(x) - 1.0), min=0), max=1.0e6).to(torch.int32)  # fp32 torch; capped as the kernel caps
    v = torch.exp(x.double()) - 1.0
    half = torch.floor(v) + 0.5
    near_half = (v - half).abs() <= DUR_HALF_REL * half.abs()
    exact = torch.clamp(torch.clamp(torch.round(v), min=0), max=1.0e6).to(torch.int32)  # half to even on the float64 value
    return SimpleNamespace(x=x, want=want, near_half=near_half, exact=exact)


def run_duration(ops, to):
    c = duration_case()
    d = to(torch.full((DUR_N,), -5, dtype=torch.int32))
    ops.duration_from_log(to(c.x), d)
    return d


def check_duration(d):
    """-> how many mismatches with the fp32 torch reference were excused as lying next to a half."""
    c = duration_case()
    assert int(c.near_half.sum()) <= DUR_EXCUSED_MAX
    wrong = host(d) != c.want
    assert not bool((wrong & ~c.near_half).any()), f"durations differ away from a half at x = {c.x[wrong & ~c.near_half][:8].tolist()}"
    return int(wrong.sum())


# ---------------------------------------------------------------------------------------------------------------------------
# 4. Glow inverse mix
# ---------------------------------------------------------------------------------------------------------------------------
GLOW_ROWS, GLOW_C = [77, 13107, 13108, 14000], 160


def glow_mix_f64(x, winv, bias, logs):
    """InvConvNear reverse then ActNorm reverse on x [rows, c], as oracle.postflow writes them (Glow.py:102-127, 30-31)."""
    c, t = x.shape[1], x.shape[0]
    y = x.t().reshape(2, c // 4, 2, t).permute(0, 2, 1, 3).reshape(4, c // 4, t)
    y = torch.einsum("on,ngt->ogt", winv.reshape(4, 4), y)
    z = y.reshape(2, 2, c // 4, t).permute(0, 2, 1, 3).reshape(c, t)
    return ((z - bias[:, None]) * torch.exp(-logs[:, None])).t()


@functools.lru_cache(maxsize=None)
def glow_case(rows):
    c = SimpleNamespace(x=as32(rnd(rows, GLOW_C, seed=1)), winv=as32(rnd(16, seed=2)), bias=as32(rnd(GLOW_C, seed=3, scale=0.1)),
                        logs=as32(rnd(GLOW_C, seed=4, scale=0.1)))
    c.want = glow_mix_f64(c.x, c.winv, c.bias, c.logs)
    return c


def run_glow(ops, to, rows, pad=0):
    """In place on a [rows, 160] view of a [rows, 160 + pad] buffer whose other columns hold the sentinel."""
    c = glow_case(rows)
    buf = torch.full((rows, GLOW_C + pad), SENTINEL, dtype=torch.float64)
    buf[:, :GLOW_C] = c.x
    buf = to(buf)
    ops.glow_invconv_actnorm(buf[:, :GLOW_C], rows, GLOW_C, to(c.winv), to(c.bias), to(c.logs))
    return buf


def check_glow(buf, rows):
    buf = host(buf)
    assert (buf[:, GLOW_C:] == SENTINEL).all(), "padding columns were written"
    return max_err(buf[:, :GLOW_C], glow_case(rows).want, TOL32, f"{rows} rows:")


# ---------------------------------------------------------------------------------------------------------------------------
# 5. depthwise conv + swish
# ---------------------------------------------------------------------------------------------------------------------------
DW_LENGTHS = [1, 2, 15, 16, 63, 64, 65, 700]
DW_CASES = [(k, c, family) for k in (7, 31) for c in (192, 80) for family in ("normal", "saturating")]


@functools.lru_cache(maxsize=None)
def dwconv_case(k, c, family):
    rag = Ragged(DW_LENGTHS, "cpu", align=2)
    w, b = as32(rnd(k, c, seed=2, scale=0.3)), as32(rnd(c, seed=3, scale=0.1))
    if family == "normal":
        x = rnd(rag.total_rows, c, seed=1)
    else:  # pre-activation standard deviation ~33 around an offset: it spans roughly +-100, the swish saturates on both sides
        x = 5.0 + rnd(rag.total_rows, c, seed=1, scale=33.0 / (0.3 * math.sqrt(k)))
    x = as32(x)
    want = []
    for b0, n in zip(rag.begins, rag.lengths):
        a = F.conv1d(x[b0:b0 + n].t().unsqueeze(0), w.t().unsqueeze(1), b, padding=(k - 1) // 2, groups=c)[0].t()
        want.append(a * torch.sigmoid(a))
    if family == "saturating":
        lo, hi = min(float(v.min()) for v in want), max(float(v.max()) for v in want)
        assert hi > 80.0 and any(bool((v == 0).any() or (v.abs() < 1e-30).any()) for v in want), (lo, hi)
    return SimpleNamespace(x=x, w=w, b=b, want=want, begins=rag.begins, rows=rag.total_rows)


def run_dwconv(ops, to, k, c, family):
    cs = dwconv_case(k, c, family)
    rag = Ragged(DW_LENGTHS, ops.device, align=2)
    y = to(torch.full((cs.rows, c), SENTINEL))
    return ops.dwconv_swish(to(cs.x), y, to(cs.w), to(cs.b), c, k, rag)


def check_dwconv(y, k, c, family):
    cs = dwconv_case(k, c, family)
    y = host(y)
    worst = 0.0
    inside = torch.zeros(cs.rows, dtype=torch.bool)
    for b0, n, want in zip(cs.begins, DW_LENGTHS, cs.want):
        inside[b0:b0 + n] = True
        worst = max(worst, max_err(y[b0:b0 + n], want, TOL32, f"{n} frames:"))
    assert (y[~inside] == SENTINEL).all()
    return worst


# ---------------------------------------------------------------------------------------------------------------------------
# 7. MAS
# ---------------------------------------------------------------------------------------------------------------------------
MAS_SHAPES = [(700, 257), (640, 321), (900, 300), (2500, 1000), (9000, 8192)]  # (T, L)
MAS_SCALES = [0.1, 1.0, 1.0, 5.0, 1.0]
MAS_FLAGGED = 2  # the L = 300 case also runs with word-boundary and repeat flags
MAS_REL = 1e-6


def viterbi_optimum_f64(pred_max):
    """The best float64 score of any monotonic path from (frame 0, token 0) to (frame T - 1, token L - 1), each frame staying on its
    token or moving to the next; scores as mas_float64_score forms them."""
    p = np.asarray(pred_max, dtype=np.float32)
    off = float(np.abs(p).max()) + 1.0
    best = np.full(p.shape[1], -np.inf)
    best[0] = np.log(np.float64(p[0, 0]) + off)
    for i in range(1, p.shape[0]):
        best = np.log(p[i].astype(np.float64) + off) + np.maximum(best, np.concatenate([[-np.inf], best[:-1]]))
    return float(best[-1])


@functools.lru_cache(maxsize=None)
def mas_case(i):
    (T, L), scale = MAS_SHAPES[i], MAS_SCALES[i]
    rng = np.random.default_rng(700 + i)
    logits = (rng.standard_normal((T, 145), dtype=np.float32) * np.float32(scale)).astype(np.float32)
    ids = rng.integers(0, 144, L).astype(np.int32)
    pm = logits[:, ids]
    dur = ar.mas(pm, log64=True)[0]
    c = SimpleNamespace(logits=logits, ids=ids, dur=dur, optimum=viterbi_optimum_f64(pm), score=ar.mas_float64_score(pm, dur))
    if i == MAS_FLAGGED:
        frng = np.random.default_rng(3)
        lf = L + L // 4
        f = np.zeros(lf, np.int32)
        f[1 + frng.choice(lf - 1, L // 4, replace=False)] |= 1  # (the first token is never a boundary)
        f[1:][frng.random(lf - 1) < 0.4] |= 2
        c.flags, c.dur_flagged = f, ar.postprocess(dur, f)
    return c


def mas_rel_gap(score, optimum):
    return abs(score - optimum) / abs(optimum)


# ---------------------------------------------------------------------------------------------------------------------------
# 9. CTC
# ---------------------------------------------------------------------------------------------------------------------------
CTC_SHAPES = [(2300, 2048), (4200, 2048), (1300, 1250), (50, 0), (1, 1), (1, 0), (2047, 2048)]  # (T, n); the last is infeasible
CTC_BLANK = 144


@functools.lru_cache(maxsize=None)
def ctc_case(i):
    T, n = CTC_SHAPES[i]
    rng = np.random.default_rng(900 + i)
    logits = rng.normal(0.0, 3.0, size=(T, 145)).astype(np.float32)
    ids = rng.integers(0, 144, size=n).astype(np.int32)
    if n > 4:
        ids[2] = ids[1]  # a repeat: needs a blank between its two labels
    return SimpleNamespace(logits=logits, ids=ids, ref32=float(sr.ctc_loss(sr.log_softmax32(logits), ids)), ref64=ctc_torch_f64(logits, ids))


def ctc_torch_f64(logits, ids):
    """torch's CTC on a float64 log-softmax, zero_infinity, / max(n, 1)."""
    lp = torch.log_softmax(torch.from_numpy(np.asarray(logits, dtype=np.float32)).double(), dim=1).unsqueeze(1)
    tg = torch.from_numpy(np.asarray(ids, dtype=np.int64)).reshape(1, -1)
    nll = F.ctc_loss(lp, tg, [lp.shape[0]], [tg.shape[1]], blank=CTC_BLANK, reduction="sum", zero_infinity=True)
    return float(nll) / max(tg.shape[1], 1)
