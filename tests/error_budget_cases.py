"""The cases of the error-budget tests (tests/error_budget.py): one table for the CPU conditions (tests/test_error_budget_cpu.py)
and the GPU run (tests/test_gpu_error_budget.py).

A case knows how to make its inputs from a seed, how to run its kernel through engine.Ops (the GPU library or the rounding model
tests/abi_emulator.py - the same call), and the plain float64 restatement of the operation.  Lengths are never written down: they
are built (`budget_lengths`) from the tile rows the launch itself uses - recorded from the descriptor engine.Ops hands to the
library (tts_conv1d_tile_rows / tts_conv1d_small_tile_rows / tts_resblock_tile_rows through packing and engine; the wide form's
selector and the WaveNet layer's tile rows as engine.Ops passes them) - and from the case's reach: 1, 2, one row short of a tile,
one row past it, and as many utterances of one tile boundary each as it takes for every row class to hold 64 rows (N_MIN
elements in every 32-channel block).

Reach: the sum of the convs' half-widths times their dilation, plus 6 for each anti-aliased snake.  tts_ffn_fused (no tile table,
no coupling between rows) and tts_relpos_attention_f16 (reach 0: no neighbourhood of an edge or a seam; the lengths are the
issue's) carry one row class, `interior`; their strata are the channel blocks.

SEED_SPREAD: s = (max - min) / mean of E_e over 8 input seeds, per case and format, measured on the CPU from the rounding model
alone with the weights and parameters fixed (tests/test_error_budget_cpu.py recomputes it and checks the table).  The margin of a
case is m = max(0.10, 3 s): 0.10 everywhere except the two attention families whose scores are made steep on purpose (rising
m = 0.36, position m = 0.33: how much probability mass is rounded at all depends on the draw).

Not in the table: attention_inputs' `peaked` family.  Every query attends to one key alone, the probabilities are 1 and 0, nothing
is rounded, and E_e / rms(r) is 1e-11 - below fp32's own resolution (MIN_REL_BUDGET), so there is no 16-bit budget to hold the
kernel to; test_relpos_attention_vs_float64 keeps covering it.

Levels (the second half of this file; tests/dynamic_range.py): `inputs(..., level=(k, da))` multiplies every additive input of the
unit-level draw by 2^k in float64 before it is stored, and adds da to every snake log alpha; weights, beta, the filters, q, k and
the position table stay.  LEVEL_CASES run at the levels of `levels(case, fmt)`; RANGE_TABLE and LEVEL_SPREAD are measured from
the model alone and recomputed by tests/test_dynamic_range_cpu.py.
"""
import contextlib
import math

import numpy as np
import torch
import torch.nn.functional as F

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import capi, engine, packing
from ims_toucan_prosody_variance_amd.ragged import Ragged
from oracle import toucan_oracle as oracle
from tests import abi_emulator, error_budget as eb, glow_ref
from tests import test_gpu_kernels_vs_float64 as vs64

COMPUTE = {"bf16": capi.COMPUTE_BF16, "f16": capi.COMPUTE_F16}
DT16 = {"bf16": torch.bfloat16, "f16": torch.float16}
ROWS_ONLY_INTERIOR = (eb.INTERIOR,)
ALL_CLASSES = (eb.EDGE, eb.SEAM, eb.INTERIOR)


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


UNIT_LEVEL = (0, 0)


def level_scale(level):
    """A level (k, da) -> (g, da) in float64: g = 2^k multiplies every additive input of a case's unit-level draw before it is stored
    in the case's storage type, da is added to every snake log alpha.  (0, 0): times 1.0 and plus 0.0, the draw bit for bit."""
    k, da = level
    return 2.0 ** int(k), float(da)


class Recording(abi_emulator.Emulator):
    """The rounding model, noting the tile rows of every launch descriptor it is handed."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.tile_rows = []

    def tts_conv1d(self, dref, stream):
        self.tile_rows.append(int(dref._obj.tile_rows))
        return super().tts_conv1d(dref, stream)

    def tts_resblock_step(self, dref, stream):
        self.tile_rows.append(int(dref._obj.tile_rows))
        return super().tts_resblock_step(dref, stream)

    def tts_wavenet_layer(self, dref, stream):
        self.tile_rows.append(int(dref._obj.tile_rows))
        return super().tts_wavenet_layer(dref, stream)


def budget_lengths(tile, reach, rows_needed=eb.N_MIN // eb.BLOCK):
    """[1, 2, tile - 1, tile + 1] and utterances with one tile boundary, both edges and interior rows between them, until the edge,
    the seam and the interior rows each number `rows_needed`."""
    per = 2 * (reach + 1)
    lengths = [1, 2, tile - 1, tile + 1]
    body = tile + 2 * per + 5
    while True:
        cls = eb.row_classes(lengths, tile, reach)
        if all(int((cls == c).sum()) >= rows_needed for c in ALL_CLASSES):
            return lengths
        lengths.append(body)
        body += 1  # (odd and even lengths: the packed layout aligns utterances to two rows)
        assert len(lengths) < 64


class Case:
    kernel = ""
    reach = 0
    channels = 0
    classes = ALL_CLASSES
    formats = ("bf16", "f16")
    model = {}          # options of the rounding model (abi_emulator.Emulator) this kernel form follows
    fixed_lengths = None

    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return self.name

    # -- shape ---------------------------------------------------------------------------------------------------------------
    def tile_rows(self, fmt):
        """The tile rows of this case's launch: a two-row utterance through engine.Ops, read off the descriptor."""
        if self.classes == ROWS_ONLY_INTERIOR:
            return None
        lib = Recording(**self.model)
        ops = engine.Ops("cpu", lib=lib)
        self.run(ops, lambda t: t.clone().contiguous(), fmt, self.inputs(fmt, 0, [2]), [2])
        assert len(set(lib.tile_rows)) == 1, lib.tile_rows
        return lib.tile_rows[0]

    def lengths(self, fmt):
        if self.fixed_lengths is not None:
            return list(self.fixed_lengths)
        return budget_lengths(self.tile_rows(fmt), self.reach)

    # -- to be provided ------------------------------------------------------------------------------------------------------
    def inputs(self, fmt, seed, lengths, level=UNIT_LEVEL):
        raise NotImplementedError

    def run(self, ops, to, fmt, inp, lengths):
        """-> the output tensor [packed rows, channels]."""
        raise NotImplementedError

    def ref(self, fmt, inp, lengths):
        """-> float64 numpy [live rows, channels]."""
        raise NotImplementedError


def layout(lengths):
    return Ragged(lengths, "cpu", align=2)


def live_rows(lengths):
    rag = layout(lengths)
    return torch.cat([torch.arange(b, b + n) for b, n in zip(rag.begins, rag.lengths)])


def spans(lengths):
    rag = layout(lengths)
    return list(zip(rag.begins, rag.lengths))


def model_ops(case, lib_class=abi_emulator.Emulator, **kw):
    return engine.Ops("cpu", lib=lib_class(**dict(case.model, **kw)))


def run_live(case, ops, fmt, inp, lengths):
    """The case on `ops` (the GPU library or a host model) -> float64 numpy [live rows, channels]."""
    on_gpu = ops.device.type == "cuda"
    to = (lambda t: t.to(ops.device).contiguous()) if on_gpu else (lambda t: t.clone().contiguous())
    out = case.run(ops, to, fmt, inp, lengths)
    if on_gpu:
        torch.cuda.synchronize()
    return out.detach().cpu()[live_rows(lengths)].double().numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# tts_conv1d
# ---------------------------------------------------------------------------------------------------------------------------------
class ConvCase(Case):
    kernel = "tts_conv1d"

    def __init__(self, name, cin, cout, k, dil, mode=capi.MODE_LINEAR, form="regular", pre=capi.PRE_NONE, io16=False, preadd=False, filt=None):
        super().__init__(name)
        self.cin, self.cout, self.k, self.dil, self.mode, self.form, self.pre, self.io16, self.preadd = cin, cout, k, dil, mode, form, pre, io16, preadd
        self.filt = filt
        self.dual = mode != capi.MODE_LINEAR
        self.channels = cout // 2 if self.dual else cout
        self.reach = (k - 1) // 2 * dil + (6 if pre == capi.PRE_SNAKE else 0)

    def inputs(self, fmt, seed, lengths, level=UNIT_LEVEL):
        s = 100 * seed
        g, da = level_scale(level)
        R = layout(lengths).total_rows
        cin, co = self.cin, self.channels
        store = (lambda t: t.to(DT16[fmt])) if self.io16 else (lambda t: t.float())
        inp = dict(w=rnd(self.cout, cin, self.k, seed=1, scale=1.0 / math.sqrt(cin * self.k)).float(), b=(g * rnd(self.cout, seed=2, scale=0.1)).float(),
                   x=store(g * rnd(R, cin, seed=s + 3)), res=store(g * rnd(R, co, seed=s + 5)))
        if self.preadd:
            inp["preadd"] = (g * rnd(R, self.cout, seed=s + 6, scale=0.5)).float()
        if self.pre == capi.PRE_SNAKE:
            inp["alpha"], inp["beta"] = (rnd(cin, seed=7, scale=0.3) + da).float(), rnd(cin, seed=8, scale=0.3).float()
            inp["filt"] = torch.from_numpy(np.ascontiguousarray(vs64.FILTERS[self.filt]()))
        return inp

    def run(self, ops, to, fmt, inp, lengths):
        rag = Ragged(lengths, ops.device, align=2)
        cw = packing.pack_conv(inp["w"].numpy(), inp["b"].numpy(), ops.device, dil=self.dil, mode=self.mode, bf16=fmt)
        tile = {"regular": cw.tile_rows, "small": cw.small_tile_rows, "wide": 256}[self.form]  # (256: the API's selector of the wide form)
        assert tile, "this shape has no such form"
        y = to(torch.zeros(rag.total_rows, self.channels, dtype=DT16[fmt] if self.io16 else torch.float32))
        snake = (to(inp["alpha"]), to(inp["beta"]), to(inp["filt"])) if self.pre == capi.PRE_SNAKE else None
        ops.conv(cw, to(inp["x"]), y, rag, pre=self.pre, pre_slope=0.1, snake=snake, res=to(inp["res"]),
                 preadd=to(inp["preadd"]) if self.preadd else None, compute=COMPUTE[fmt], tile_rows=tile)
        return y

    def ref(self, fmt, inp, lengths):
        w, b, co = inp["w"].double(), inp["b"].double(), self.channels
        out = []
        for b0, n in spans(lengths):
            x = inp["x"][b0:b0 + n].double()
            if self.pre == capi.PRE_LRELU:
                x = F.leaky_relu(x, float(np.float32(0.1)))
            if self.pre == capi.PRE_SNAKE:
                t = vs64.snake_f64(x, inp["alpha"].double(), inp["beta"].double(), inp["filt"].double()).unsqueeze(0)
            else:
                t = x.t().unsqueeze(0)
            a = F.conv1d(t, w, b, padding=(self.k - 1) // 2 * self.dil, dilation=self.dil)[0].t()
            if self.preadd:
                a = a + inp["preadd"][b0:b0 + n].double()
            if self.mode == capi.MODE_GLU:
                a = a[:, :co] * torch.sigmoid(a[:, co:])
            elif self.mode == capi.MODE_GATED:
                a = torch.tanh(a[:, :co]) * torch.sigmoid(a[:, co:])
            out.append(a + inp["res"][b0:b0 + n].double())
        return torch.cat(out).numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# tts_resblock_step
# ---------------------------------------------------------------------------------------------------------------------------------
class ResblockCase(Case):
    kernel = "tts_resblock_step"

    def __init__(self, name, c, k, dil, act, io16=False, filt="design", model=None):
        super().__init__(name)
        self.c, self.k, self.dil, self.act, self.io16, self.filt = c, k, dil, act, io16, filt
        self.channels = c
        h = (k - 1) // 2
        self.reach = h * dil + h + (12 if act == capi.PRE_SNAKE else 0)
        self.model = model or {}

    def inputs(self, fmt, seed, lengths, level=UNIT_LEVEL):
        s, c, k = 100 * seed, self.c, self.k
        g, da = level_scale(level)
        R = layout(lengths).total_rows
        x = g * rnd(R, c, seed=s + 5)
        return dict(w1=rnd(c, c, k, seed=1, scale=1.0 / math.sqrt(c * k)).float(), w2=rnd(c, c, k, seed=2, scale=1.0 / math.sqrt(c * k)).float(),
                    b1=(g * rnd(c, seed=3, scale=0.1)).float(), b2=(g * rnd(c, seed=4, scale=0.1)).float(),
                    x=x.to(DT16[fmt]) if self.io16 else x.float(),
                    a1=(rnd(c, seed=7, scale=0.3) + da).float(), be1=rnd(c, seed=8, scale=0.3).float(),
                    a2=(rnd(c, seed=9, scale=0.3) + da).float(), be2=rnd(c, seed=10, scale=0.3).float(),
                    filt=torch.from_numpy(np.ascontiguousarray(vs64.FILTERS[self.filt]())))

    def run(self, ops, to, fmt, inp, lengths):
        rag = Ragged(lengths, ops.device, align=2)
        c1 = packing.pack_conv(inp["w1"].numpy(), inp["b1"].numpy(), ops.device, dil=self.dil, bf16=fmt)
        c2 = packing.pack_conv(inp["w2"].numpy(), inp["b2"].numpy(), ops.device, dil=1, bf16=fmt)
        x = to(inp["x"])
        y = torch.zeros_like(x)
        filt = to(inp["filt"])
        return ops.resblock_step(c1, c2, x, y, rag, self.act, 0.1, (to(inp["a1"]), to(inp["be1"])), (to(inp["a2"]), to(inp["be2"])), filt,
                                 fir_tab=packing.snake_fir_table(inp["filt"].numpy(), ops.device))

    def ref(self, fmt, inp, lengths):
        w1, w2, b1, b2, f = (inp[n].double() for n in ("w1", "w2", "b1", "b2", "filt"))
        pad = (self.k - 1) // 2
        slope = float(np.float32(0.1))
        out = []
        for b0, n in spans(lengths):
            x = inp["x"][b0:b0 + n].double()
            if self.act == capi.PRE_SNAKE:
                t = F.conv1d(vs64.snake_f64(x, inp["a1"].double(), inp["be1"].double(), f).unsqueeze(0), w1, b1, padding=pad * self.dil, dilation=self.dil)
                t = oracle.activation1d(t[0], lambda v: oracle.snake_beta(v, inp["a2"].double(), inp["be2"].double()), f).unsqueeze(0)
            else:
                t = F.conv1d(F.leaky_relu(x, slope).t().unsqueeze(0), w1, b1, padding=pad * self.dil, dilation=self.dil)
                t = F.leaky_relu(t, slope)
            out.append(F.conv1d(t, w2, b2, padding=pad)[0].t() + x)
        return torch.cat(out).numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# tts_wavenet_layer
# ---------------------------------------------------------------------------------------------------------------------------------
class WavenetCase(Case):
    kernel = "tts_wavenet_layer"
    reach = 2
    H = 192

    def __init__(self, name, cout2):
        super().__init__(name)
        self.cout2 = self.channels = cout2

    def inputs(self, fmt, seed, lengths, level=UNIT_LEVEL):
        s, H = 100 * seed, self.H
        g, _ = level_scale(level)
        R = layout(lengths).total_rows
        return dict(w_in=rnd(2 * H, H, 5, seed=1, scale=1.0 / math.sqrt(5 * H)).float(), b_in=(g * rnd(2 * H, seed=2, scale=0.1)).float(),
                    w_rs=rnd(self.cout2, H, 1, seed=3, scale=1.0 / math.sqrt(H)).float(), b_rs=(g * rnd(self.cout2, seed=4, scale=0.1)).float(),
                    hs=(g * rnd(R, 2 * H, seed=s + 5)).float(), cond=(g * rnd(R, 8 * H, seed=s + 6, scale=0.5)).float())

    def run(self, ops, to, fmt, inp, lengths):
        H = self.H
        rag = Ragged(lengths, ops.device, align=2)
        inl = packing.pack_conv(inp["w_in"].numpy(), inp["b_in"].numpy(), ops.device, mode=capi.MODE_GATED, bf16=fmt)
        rs = packing.pack_conv(inp["w_rs"].numpy(), inp["b_rs"].numpy(), ops.device, bf16=fmt)
        cond = to(inp["cond"])[:, 2 * H:4 * H]  # a 384-column slice of the [R, 1536] conditioning
        out = to(torch.zeros(rag.total_rows, 2 * H))
        ops.wavenet_layer(inl, rs, to(inp["hs"]), out, cond, rag)
        return out if self.cout2 == 2 * H else out[:, H:]

    def ref(self, fmt, inp, lengths):
        H = self.H
        out = []
        for b0, n in spans(lengths):
            hs, cond = inp["hs"][b0:b0 + n].double().numpy(), inp["cond"][b0:b0 + n, 2 * H:4 * H].double().numpy()
            a = glow_ref.conv1d(hs[:, :H], inp["w_in"].numpy(), inp["b_in"].numpy()) + cond
            with np.errstate(over="ignore"):  # (a gate of a few thousand at the upper levels: e^-a = inf, the sigmoid 0)
                acts = np.tanh(a[:, :H]) / (1.0 + np.exp(-a[:, H:]))
            rs = glow_ref.conv1d(acts, inp["w_rs"].numpy(), inp["b_rs"].numpy())
            out.append((hs if self.cout2 == 2 * H else hs[:, H:]) + rs)
        return np.concatenate(out)


# ---------------------------------------------------------------------------------------------------------------------------------
# tts_ffn_fused
# ---------------------------------------------------------------------------------------------------------------------------------
class FfnCase(Case):
    kernel = "tts_ffn_fused"
    classes = ROWS_ONLY_INTERIOR
    channels = 192

    def __init__(self, name, rows, hidden, post):
        super().__init__(name)
        self.hidden, self.post = hidden, post
        self.fixed_lengths = [rows]

    def inputs(self, fmt, seed, lengths, level=UNIT_LEVEL):
        s, C, hid = 100 * seed, 192, self.hidden
        g, _ = level_scale(level)
        return dict(w1=rnd(hid, C, 1, seed=1, scale=1.0 / math.sqrt(C)).float(), b1=rnd(hid, seed=2, scale=0.1).float(),
                    w2=rnd(C, hid, 1, seed=3, scale=1.0 / math.sqrt(hid)).float(), b2=rnd(C, seed=4, scale=0.1).float(),
                    x=(g * rnd(lengths[0], C, seed=s + 5, scale=2.0)).float(),
                    g=(1.0 + rnd(C, seed=6, scale=0.1)).float(), b=rnd(C, seed=7, scale=0.1).float(),
                    pg=(1.0 + rnd(C, seed=8, scale=0.1)).float(), pb=rnd(C, seed=9, scale=0.1).float())

    def run(self, ops, to, fmt, inp, lengths):
        rows = lengths[0]
        x = to(inp["x"])
        c2 = packing.pack_conv(inp["w2"].numpy(), inp["b2"].numpy(), ops.device, bf16=fmt)
        pk = packing.pack_ffn(inp["w1"].numpy(), inp["b1"].numpy(), inp["w2"].numpy(), ops.device, fmt)
        post = (to(inp["pg"]), to(inp["pb"])) if self.post else None
        return ops.ffn_fused(x, x, (to(inp["g"]), to(inp["b"])), pk, c2.bias, rows, COMPUTE[fmt], post=post)

    def ref(self, fmt, inp, lengths):
        d = {k: v.double() for k, v in inp.items()}
        sd = {"w_1.weight": d["w1"], "w_1.bias": d["b1"], "w_2.weight": d["w2"], "w_2.bias": d["b2"]}
        y = d["x"] + 0.5 * oracle.ffn(oracle.layer_norm(d["x"], d["g"], d["b"]), sd, "")
        if self.post:
            y = oracle.layer_norm(y, d["pg"], d["pb"])
        return y.numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# tts_relpos_attention_f16
# ---------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _seeds_shifted(by):
    """attention_inputs draws from fixed seeds: shift those of q, k and v (seeds 1 to 3) for the seed spread."""
    orig = vs64.rnd
    vs64.rnd = lambda *shape, seed=0, scale=1.0: orig(*shape, seed=seed + by if seed in (1, 2, 3) else seed, scale=scale)
    try:
        yield
    finally:
        vs64.rnd = orig


class AttentionCase(Case):
    kernel = "tts_relpos_attention_f16"
    classes = ROWS_ONLY_INTERIOR
    channels = vs64.HD
    formats = ("f16",)

    def __init__(self, name, lengths, family, place=None):
        super().__init__(name)
        self.fixed_lengths, self.family, self.place = lengths, family, place

    def inputs(self, fmt, seed, lengths, level=UNIT_LEVEL):
        with _seeds_shifted(100 * seed):
            qkv, ptab, bu, bv = vs64.attention_inputs(self.family, layout(lengths), self.place)
        qkv = torch.cat([qkv[:, :2 * vs64.HD], level_scale(level)[0] * qkv[:, 2 * vs64.HD:]], 1)  # (the v third alone)
        return dict(qkv=qkv.float(), ptab=ptab.float(), bu=bu.float(), bv=bv.float())

    def run(self, ops, to, fmt, inp, lengths):
        rag = Ragged(lengths, ops.device, align=2)
        ctx = to(torch.zeros(rag.total_rows, vs64.HD))
        return ops.attention(to(inp["qkv"]), to(inp["ptab"]), vs64.PMAX, to(inp["bu"]), to(inp["bv"]), ctx, rag, f16=True)

    def ref(self, fmt, inp, lengths):
        d = {k: v.double() for k, v in inp.items()}
        return torch.cat([vs64.attention_f64(d["qkv"][b0:b0 + n], d["ptab"], vs64.PMAX, d["bu"], d["bv"], n) for b0, n in spans(lengths)]).numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# The table
# ---------------------------------------------------------------------------------------------------------------------------------
LRELU, SNAKE = capi.PRE_LRELU, capi.PRE_SNAKE
MFMA = dict(mfma_snake=True)  # the matrix-core snake's rounding points (abi_emulator.Emulator's option)

CASES = [
    ConvCase("conv regular linear 192>256 k5", 192, 256, 5, 1),
    ConvCase("conv small glu 192>2x192 k3 d2", 192, 384, 3, 2, mode=capi.MODE_GLU, form="small"),
    ConvCase("conv small gated 192>2x192 k5 preadd", 192, 384, 5, 1, mode=capi.MODE_GATED, form="small", preadd=True),
    ConvCase("conv regular lrelu 64>64 k11 d5 16-bit hbm", 64, 64, 11, 5, pre=LRELU, io16=True),
    ConvCase("conv small lrelu 96>128 k7 d3", 96, 128, 7, 3, pre=LRELU, form="small"),
    ConvCase("conv wide 256>256 k7 d3 16-bit hbm", 256, 256, 7, 3, form="wide", io16=True),
    ConvCase("conv snake 32>32 k3", 32, 32, 3, 1, pre=SNAKE, filt="design"),
    ConvCase("conv snake 128>128 k11 d5 asymmetric", 128, 128, 11, 5, pre=SNAKE, filt="asymmetric"),
    ConvCase("conv snake 256>256 k7 d3 stored", 256, 256, 7, 3, pre=SNAKE, filt="stored"),
    ResblockCase("resblock lrelu 64 k7 d3", 64, 7, 3, LRELU),
    ResblockCase("resblock lrelu 128 k3 16-bit stream", 128, 3, 1, LRELU, io16=True),
    ResblockCase("resblock mfma snake 32 k3 16-bit stream", 32, 3, 1, SNAKE, io16=True, model=MFMA),
    ResblockCase("resblock mfma snake 64 k7 d3 asymmetric", 64, 7, 3, SNAKE, filt="asymmetric", model=MFMA),
    ResblockCase("resblock mfma snake 128 k11 d5 stored", 128, 11, 5, SNAKE, filt="stored", model=MFMA),
    ResblockCase("resblock valu snake 256 k3 16-bit stream", 256, 3, 1, SNAKE, io16=True, filt="asymmetric"),
    WavenetCase("wavenet layer cout2 384", 384),
    WavenetCase("wavenet last layer cout2 192", 192),
    FfnCase("ffn 1536 post 300 rows", 300, 1536, True),
    FfnCase("ffn 1536 no post 129 rows", 129, 1536, False),
    FfnCase("ffn 64 post 301 rows", 301, 64, True),
    FfnCase("ffn 64 no post 257 rows", 257, 64, False),
    AttentionCase("attention gentle [129, 31, 33]", [129, 31, 33], "gentle"),
    AttentionCase("attention rising [129, 31, 33]", [129, 31, 33], "rising"),
    AttentionCase("attention position [129, 31, 33]", [129, 31, 33], "position"),
    AttentionCase("attention gentle [640]", [640], "gentle"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# A budget this close to fp32's own resolution is no budget: the kernels' fp32 epilogues are not part of the 16-bit rounding model.
MIN_REL_BUDGET = 2.0 ** -17

# s of every (case, format): the rounding model alone on 8 input seeds (weights and parameters fixed)
SEED_SPREAD = {
    ("conv regular linear 192>256 k5", "bf16"): 0.0050,
    ("conv regular linear 192>256 k5", "f16"): 0.0060,
    ("conv small glu 192>2x192 k3 d2", "bf16"): 0.0051,
    ("conv small glu 192>2x192 k3 d2", "f16"): 0.0051,
    ("conv small gated 192>2x192 k5 preadd", "bf16"): 0.0089,
    ("conv small gated 192>2x192 k5 preadd", "f16"): 0.0072,
    ("conv regular lrelu 64>64 k11 d5 16-bit hbm", "bf16"): 0.0147,
    ("conv regular lrelu 64>64 k11 d5 16-bit hbm", "f16"): 0.0179,
    ("conv small lrelu 96>128 k7 d3", "bf16"): 0.0190,
    ("conv small lrelu 96>128 k7 d3", "f16"): 0.0172,
    ("conv wide 256>256 k7 d3 16-bit hbm", "bf16"): 0.0050,
    ("conv wide 256>256 k7 d3 16-bit hbm", "f16"): 0.0053,
    ("conv snake 32>32 k3", "bf16"): 0.0137,
    ("conv snake 32>32 k3", "f16"): 0.0175,
    ("conv snake 128>128 k11 d5 asymmetric", "bf16"): 0.0133,
    ("conv snake 128>128 k11 d5 asymmetric", "f16"): 0.0163,
    ("conv snake 256>256 k7 d3 stored", "bf16"): 0.0073,
    ("conv snake 256>256 k7 d3 stored", "f16"): 0.0064,
    ("resblock lrelu 64 k7 d3", "bf16"): 0.0093,
    ("resblock lrelu 64 k7 d3", "f16"): 0.0077,
    ("resblock lrelu 128 k3 16-bit stream", "bf16"): 0.0097,
    ("resblock lrelu 128 k3 16-bit stream", "f16"): 0.0039,
    ("resblock mfma snake 32 k3 16-bit stream", "bf16"): 0.0179,
    ("resblock mfma snake 32 k3 16-bit stream", "f16"): 0.0239,
    ("resblock mfma snake 64 k7 d3 asymmetric", "bf16"): 0.0116,
    ("resblock mfma snake 64 k7 d3 asymmetric", "f16"): 0.0058,
    ("resblock mfma snake 128 k11 d5 stored", "bf16"): 0.0174,
    ("resblock mfma snake 128 k11 d5 stored", "f16"): 0.0138,
    ("resblock valu snake 256 k3 16-bit stream", "bf16"): 0.0099,
    ("resblock valu snake 256 k3 16-bit stream", "f16"): 0.0069,
    ("wavenet layer cout2 384", "bf16"): 0.0068,
    ("wavenet layer cout2 384", "f16"): 0.0055,
    ("wavenet last layer cout2 192", "bf16"): 0.0075,
    ("wavenet last layer cout2 192", "f16"): 0.0060,
    ("ffn 1536 post 300 rows", "bf16"): 0.0146,
    ("ffn 1536 post 300 rows", "f16"): 0.0142,
    ("ffn 1536 no post 129 rows", "bf16"): 0.0167,
    ("ffn 1536 no post 129 rows", "f16"): 0.0150,
    ("ffn 64 post 301 rows", "bf16"): 0.0269,
    ("ffn 64 post 301 rows", "f16"): 0.0236,
    ("ffn 64 no post 257 rows", "bf16"): 0.0239,
    ("ffn 64 no post 257 rows", "f16"): 0.0260,
    ("attention gentle [129, 31, 33]", "f16"): 0.0225,
    ("attention rising [129, 31, 33]", "f16"): 0.1214,
    ("attention position [129, 31, 33]", "f16"): 0.1114,
    ("attention gentle [640]", "f16"): 0.0125,
}


def case_margin(case, fmt):
    return eb.margin(SEED_SPREAD[(case.name, fmt)])


def case_ids():
    return [(c, f) for c in CASES for f in c.formats]


# ---------------------------------------------------------------------------------------------------------------------------------
# Levels (tests/dynamic_range.py): the cases above away from unit scale
# ---------------------------------------------------------------------------------------------------------------------------------
# One case per kernel family and per hidden 16-bit stage, each in the formats it already has.
LEVEL_CASES = [
    "conv regular lrelu 64>64 k11 d5 16-bit hbm",
    "conv wide 256>256 k7 d3 16-bit hbm",
    "conv small gated 192>2x192 k5 preadd",
    "conv snake 128>128 k11 d5 asymmetric",
    "resblock lrelu 128 k3 16-bit stream",
    "resblock mfma snake 32 k3 16-bit stream",
    "resblock mfma snake 128 k11 d5 stored",
    "resblock valu snake 256 k3 16-bit stream",
    "wavenet layer cout2 384",
    "ffn 1536 post 300 rows",
    "attention gentle [129, 31, 33]",
]
SNAKE_LEVEL_CASES = [n for n in LEVEL_CASES if "snake" in n]
# bf16 throughout, no transcendental: a power of two commutes with every rounding of the plain model and of the kernel
HOMOGENEOUS_CASES = ["conv regular lrelu 64>64 k11 d5 16-bit hbm", "conv wide 256>256 k7 d3 16-bit hbm", "resblock lrelu 128 k3 16-bit stream"]
# What the levels showed the kernels to do that the unit-level model does not say ("The 16-bit kernels over the dynamic range"):
# options of the rounding model on top of the case's own, at every level of the case (the unit-level tests keep their model).
LEVEL_MODEL = {
    "resblock mfma snake 32 k3 16-bit stream": dict(snake_offset_sum=True),
    "resblock mfma snake 128 k11 d5 stored": dict(snake_offset_sum=True),
    "wavenet layer cout2 384": dict(fast_gate=True),
    "ffn 1536 post 300 rows": dict(f32_norms=True),
}
LEVEL_K = (-22, -18, -14, 12)
LEVEL_DA = (2, 4)
SWEEP_K = tuple(range(-26, 18))
SWEEP_DA = tuple(range(0, 6))
TABLE_K = (-22, -18, -14, 0, 12)  # the k whose E_e / rms(r) a row of RANGE_TABLE records, beside k_top's


def level_id(level):
    k, da = level
    return f"2^{k:+d}" + (f" log alpha {da:+d}" if da else "")


def level_model(case):
    """The model options of a case at its levels."""
    return dict(case.model, **LEVEL_MODEL.get(case.name, {}))


def level_case_ids():
    return [(BY_NAME[n], f) for n in LEVEL_CASES for f in BY_NAME[n].formats]


def levels(case, fmt):
    """The GPU levels of a (case, format): LEVEL_K; LEVEL_DA at k = 0 for a snake case; and one octave under the last finite scale
    of the model the kernel follows (the kernel accumulates in fp32 in its own order and may carry a sum across the format's
    largest number that the float64-accumulating model keeps just under it) unless that is one of LEVEL_K."""
    out = [(k, 0) for k in LEVEL_K]
    if case.name in SNAKE_LEVEL_CASES:
        out += [(0, da) for da in LEVEL_DA]
    top = RANGE_TABLE[(case.name, fmt, "kernel")]["k_top"] - 1
    if top not in LEVEL_K:
        out.append((top, 0))
    return out


def level_ids():
    return [(c, f, lv) for c, f in level_case_ids() for lv in levels(c, f)]


def level_margin(case, fmt, level):
    return eb.margin(LEVEL_SPREAD[(case.name, fmt, level)])
# The range of every rounding model, from the sweep of tests/dynamic_range.py (seed 0, k = -26 ... 17 at da = 0; da = 0 ... 5 at k = 0 for the
# snake cases); tests/test_dynamic_range_cpu.py recomputes every row (integers exactly, ratios to 1 %).  "kernel": the model with the
# options the case names (what the kernel does); "plain": the plain-format model (mfma_snake=False) of a case that names options.
#   k_top    the largest k such that the model is finite at every k' <= k (17: finite over the whole sweep)
#   k_floor  the smallest k at which E_e / rms(r) is at most twice its unit-level value (-26: over the whole sweep); descriptive
#   rel      E_e / rms(r) at TABLE_K and at k_top
#   da_top, da_2x, rel_da   the same over the sharpness: the last finite da, the last da up to which E_e / rms(r) stays within twice
#            the unit level's, and E_e / rms(r) at da = 0 ... 5
RANGE_TABLE = {
    ('conv regular lrelu 64>64 k11 d5 16-bit hbm', 'bf16', 'kernel'): dict(k_top=17, k_floor=-26, rel={-22: 1.903e-03, -18: 1.903e-03, -14: 1.903e-03, 0: 1.903e-03, 12: 1.903e-03, 17: 1.903e-03}),
    ('conv regular lrelu 64>64 k11 d5 16-bit hbm', 'f16', 'kernel'): dict(k_top=13, k_floor=-14, rel={-22: 7.135e-02, -18: 4.507e-03, -14: 3.321e-04, 0: 2.385e-04, 12: 2.385e-04, 13: 2.385e-04}),
    ('conv wide 256>256 k7 d3 16-bit hbm', 'bf16', 'kernel'): dict(k_top=17, k_floor=-26, rel={-22: 2.022e-03, -18: 2.022e-03, -14: 2.022e-03, 0: 2.022e-03, 12: 2.022e-03, 17: 2.022e-03}),
    ('conv wide 256>256 k7 d3 16-bit hbm', 'f16', 'kernel'): dict(k_top=13, k_floor=-15, rel={-22: 5.107e-02, -18: 3.203e-03, -14: 2.864e-04, 0: 2.529e-04, 12: 2.529e-04, 13: 2.529e-04}),
    ('conv small gated 192>2x192 k5 preadd', 'bf16', 'kernel'): dict(k_top=17, k_floor=-26, rel={-22: 1.016e-03, -18: 1.016e-03, -14: 1.016e-03, 0: 8.325e-04, 12: 9.921e-06, 17: 3.358e-07}),
    ('conv small gated 192>2x192 k5 preadd', 'f16', 'kernel'): dict(k_top=13, k_floor=-14, rel={-22: 3.128e-02, -18: 1.953e-03, -14: 1.580e-04, 0: 1.041e-04, 12: 2.763e-06, 13: 1.688e-06}),
    ('conv snake 128>128 k11 d5 asymmetric', 'bf16', 'kernel'): dict(k_top=17, k_floor=-26, rel={-22: 1.501e-03, -18: 1.501e-03, -14: 1.501e-03, 0: 1.640e-03, 12: 1.502e-03, 17: 1.501e-03}, da_top=5, da_2x=5, rel_da=[1.640e-03, 1.660e-03, 1.663e-03, 1.662e-03, 1.659e-03, 1.654e-03]),
    ('conv snake 128>128 k11 d5 asymmetric', 'f16', 'kernel'): dict(k_top=14, k_floor=-14, rel={-22: 5.223e-02, -18: 3.286e-03, -14: 2.502e-04, 0: 2.036e-04, 12: 1.892e-04, 14: 1.885e-04}, da_top=5, da_2x=5, rel_da=[2.036e-04, 2.036e-04, 2.039e-04, 2.055e-04, 2.033e-04, 2.044e-04]),
    ('resblock lrelu 128 k3 16-bit stream', 'bf16', 'kernel'): dict(k_top=17, k_floor=-26, rel={-22: 2.096e-03, -18: 2.096e-03, -14: 2.096e-03, 0: 2.096e-03, 12: 2.096e-03, 17: 2.096e-03}),
    ('resblock lrelu 128 k3 16-bit stream', 'f16', 'kernel'): dict(k_top=13, k_floor=-14, rel={-22: 9.266e-02, -18: 5.951e-03, -14: 4.149e-04, 0: 2.650e-04, 12: 2.650e-04, 13: 2.650e-04}),
    ('resblock mfma snake 32 k3 16-bit stream', 'bf16', 'kernel'): dict(k_top=13, k_floor=-17, rel={-22: 8.836e-02, -18: 6.257e-03, -14: 2.704e-03, 0: 3.026e-03, 12: 2.693e-03, 13: 2.700e-03}, da_top=5, da_2x=1, rel_da=[3.026e-03, 3.712e-03, 7.281e-03, 2.387e-02, 1.124e-01, 2.143e-01]),
    ('resblock mfma snake 32 k3 16-bit stream', 'bf16', 'plain'): dict(k_top=17, k_floor=-26, rel={-22: 2.827e-03, -18: 2.826e-03, -14: 2.832e-03, 0: 3.249e-03, 12: 2.826e-03, 17: 2.826e-03}, da_top=5, da_2x=1, rel_da=[3.249e-03, 4.030e-03, 7.871e-03, 2.009e-02, 5.313e-02, 1.257e-01]),
    ('resblock mfma snake 32 k3 16-bit stream', 'f16', 'kernel'): dict(k_top=13, k_floor=-15, rel={-22: 1.194e-01, -18: 7.605e-03, -14: 7.675e-04, 0: 7.855e-04, 12: 6.670e-04, 13: 6.588e-04}, da_top=5, da_2x=1, rel_da=[7.855e-04, 1.036e-03, 2.952e-03, 1.706e-02, 1.067e-01, 2.129e-01]),
    ('resblock mfma snake 32 k3 16-bit stream', 'f16', 'plain'): dict(k_top=13, k_floor=-14, rel={-22: 1.051e-01, -18: 6.591e-03, -14: 4.787e-04, 0: 4.003e-04, 12: 3.588e-04, 13: 3.569e-04}, da_top=5, da_2x=1, rel_da=[4.003e-04, 5.069e-04, 9.758e-04, 2.535e-03, 6.759e-03, 1.822e-02]),
    ('resblock mfma snake 128 k11 d5 stored', 'bf16', 'kernel'): dict(k_top=13, k_floor=-17, rel={-22: 8.871e-02, -18: 5.916e-03, -14: 2.159e-03, 0: 2.541e-03, 12: 2.134e-03, 13: 2.135e-03}, da_top=5, da_2x=1, rel_da=[2.541e-03, 3.320e-03, 7.277e-03, 2.685e-02, 1.378e-01, 2.209e-01]),
    ('resblock mfma snake 128 k11 d5 stored', 'bf16', 'plain'): dict(k_top=17, k_floor=-26, rel={-22: 2.267e-03, -18: 2.268e-03, -14: 2.270e-03, 0: 2.726e-03, 12: 2.272e-03, 17: 2.267e-03}, da_top=5, da_2x=1, rel_da=[2.726e-03, 3.701e-03, 7.743e-03, 1.997e-02, 5.360e-02, 1.259e-01]),
    ('resblock mfma snake 128 k11 d5 stored', 'f16', 'kernel'): dict(k_top=13, k_floor=-15, rel={-22: 1.143e-01, -18: 7.181e-03, -14: 7.470e-04, 0: 7.681e-04, 12: 6.490e-04, 13: 6.451e-04}, da_top=5, da_2x=1, rel_da=[7.681e-04, 1.084e-03, 3.538e-03, 2.166e-02, 1.342e-01, 2.199e-01]),
    ('resblock mfma snake 128 k11 d5 stored', 'f16', 'plain'): dict(k_top=13, k_floor=-14, rel={-22: 8.821e-02, -18: 5.522e-03, -14: 4.004e-04, 0: 3.478e-04, 12: 2.915e-04, 13: 2.856e-04}, da_top=5, da_2x=1, rel_da=[3.478e-04, 4.669e-04, 9.548e-04, 2.527e-03, 6.732e-03, 1.831e-02]),
    ('resblock valu snake 256 k3 16-bit stream', 'bf16', 'kernel'): dict(k_top=17, k_floor=-26, rel={-22: 2.840e-03, -18: 2.844e-03, -14: 2.840e-03, 0: 3.226e-03, 12: 2.844e-03, 17: 2.845e-03}, da_top=5, da_2x=1, rel_da=[3.226e-03, 4.134e-03, 8.233e-03, 2.106e-02, 5.546e-02, 1.333e-01]),
    ('resblock valu snake 256 k3 16-bit stream', 'f16', 'kernel'): dict(k_top=13, k_floor=-14, rel={-22: 1.036e-01, -18: 6.521e-03, -14: 4.758e-04, 0: 4.051e-04, 12: 3.609e-04, 13: 3.573e-04}, da_top=5, da_2x=1, rel_da=[4.051e-04, 5.193e-04, 1.034e-03, 2.650e-03, 7.135e-03, 1.945e-02]),
    ('wavenet layer cout2 384', 'bf16', 'kernel'): dict(k_top=17, k_floor=-16, rel={-22: 7.651e-02, -18: 4.950e-03, -14: 1.576e-03, 0: 1.148e-03, 12: 9.899e-06, 17: 3.321e-07}),
    ('wavenet layer cout2 384', 'bf16', 'plain'): dict(k_top=17, k_floor=-26, rel={-22: 1.528e-03, -18: 1.528e-03, -14: 1.528e-03, 0: 1.148e-03, 12: 9.899e-06, 17: 3.321e-07}),
    ('wavenet layer cout2 384', 'f16', 'kernel'): dict(k_top=14, k_floor=-13, rel={-22: 8.285e-02, -18: 5.155e-03, -14: 3.541e-04, 0: 1.435e-04, 12: 2.520e-06, 14: 1.313e-05}),
    ('wavenet layer cout2 384', 'f16', 'plain'): dict(k_top=14, k_floor=-13, rel={-22: 7.016e-02, -18: 4.404e-03, -14: 3.095e-04, 0: 1.435e-04, 12: 2.520e-06, 14: 1.313e-05}),
    ('ffn 1536 post 300 rows', 'bf16', 'kernel'): dict(k_top=17, k_floor=-1, rel={-22: 3.224e-03, -18: 3.399e-03, -14: 3.437e-03, 0: 5.805e-04, 12: 1.676e-07, 17: 8.713e-08}),
    ('ffn 1536 post 300 rows', 'bf16', 'plain'): dict(k_top=17, k_floor=-1, rel={-22: 3.224e-03, -18: 3.399e-03, -14: 3.437e-03, 0: 5.806e-04, 12: 1.485e-07, 17: 3.574e-08}),
    ('ffn 1536 post 300 rows', 'f16', 'kernel'): dict(k_top=17, k_floor=-1, rel={-22: 4.060e-04, -18: 4.298e-04, -14: 4.311e-04, 0: 7.277e-05, 12: 8.734e-08, 17: 8.717e-08}),
    ('ffn 1536 post 300 rows', 'f16', 'plain'): dict(k_top=17, k_floor=-1, rel={-22: 4.061e-04, -18: 4.298e-04, -14: 4.312e-04, 0: 7.279e-05, 12: 3.991e-08, 17: 3.547e-08}),
    ('attention gentle [129, 31, 33]', 'f16', 'kernel'): dict(k_top=14, k_floor=-18, rel={-22: 1.028e-01, -18: 1.856e-04, -14: 1.856e-04, 0: 1.856e-04, 12: 1.856e-04, 14: 1.856e-04}),
}

# s of every (case, format, level): measured as SEED_SPREAD is - the rounding model alone on 8 input seeds; m = max(0.10, 3 s).
# (The gated conv and the WaveNet layer at 2^12 and above: tanh and the sigmoid saturate, the 16-bit budget is spent by the few
# elements that do not, and how many there are depends on the draw.)
LEVEL_SPREAD = {
    ('conv regular lrelu 64>64 k11 d5 16-bit hbm', 'bf16', (-22, 0)): 0.0147,
    ('conv regular lrelu 64>64 k11 d5 16-bit hbm', 'bf16', (-18, 0)): 0.0147,
    ('conv regular lrelu 64>64 k11 d5 16-bit hbm', 'bf16', (-14, 0)): 0.0147,
    ('conv regular lrelu 64>64 k11 d5 16-bit hbm', 'bf16', (12, 0)): 0.0147,
    ('conv regular lrelu 64>64 k11 d5 16-bit hbm', 'bf16', (16, 0)): 0.0147,
    ('conv regular lrelu 64>64 k11 d5 16-bit hbm', 'f16', (-22, 0)): 0.0079,
    ('conv regular lrelu 64>64 k11 d5 16-bit hbm', 'f16', (-18, 0)): 0.0083,
    ('conv regular lrelu 64>64 k11 d5 16-bit hbm', 'f16', (-14, 0)): 0.0103,
    ('conv regular lrelu 64>64 k11 d5 16-bit hbm', 'f16', (12, 0)): 0.0179,
    ('conv wide 256>256 k7 d3 16-bit hbm', 'bf16', (-22, 0)): 0.0050,
    ('conv wide 256>256 k7 d3 16-bit hbm', 'bf16', (-18, 0)): 0.0050,
    ('conv wide 256>256 k7 d3 16-bit hbm', 'bf16', (-14, 0)): 0.0050,
    ('conv wide 256>256 k7 d3 16-bit hbm', 'bf16', (12, 0)): 0.0050,
    ('conv wide 256>256 k7 d3 16-bit hbm', 'bf16', (16, 0)): 0.0050,
    ('conv wide 256>256 k7 d3 16-bit hbm', 'f16', (-22, 0)): 0.0014,
    ('conv wide 256>256 k7 d3 16-bit hbm', 'f16', (-18, 0)): 0.0019,
    ('conv wide 256>256 k7 d3 16-bit hbm', 'f16', (-14, 0)): 0.0031,
    ('conv wide 256>256 k7 d3 16-bit hbm', 'f16', (12, 0)): 0.0053,
    ('conv small gated 192>2x192 k5 preadd', 'bf16', (-22, 0)): 0.0090,
    ('conv small gated 192>2x192 k5 preadd', 'bf16', (-18, 0)): 0.0090,
    ('conv small gated 192>2x192 k5 preadd', 'bf16', (-14, 0)): 0.0090,
    ('conv small gated 192>2x192 k5 preadd', 'bf16', (12, 0)): 0.1068,
    ('conv small gated 192>2x192 k5 preadd', 'bf16', (16, 0)): 0.0943,
    ('conv small gated 192>2x192 k5 preadd', 'f16', (-22, 0)): 0.0039,
    ('conv small gated 192>2x192 k5 preadd', 'f16', (-18, 0)): 0.0062,
    ('conv small gated 192>2x192 k5 preadd', 'f16', (-14, 0)): 0.0087,
    ('conv small gated 192>2x192 k5 preadd', 'f16', (12, 0)): 0.4269,
    ('conv snake 128>128 k11 d5 asymmetric', 'bf16', (-22, 0)): 0.0105,
    ('conv snake 128>128 k11 d5 asymmetric', 'bf16', (-18, 0)): 0.0098,
    ('conv snake 128>128 k11 d5 asymmetric', 'bf16', (-14, 0)): 0.0110,
    ('conv snake 128>128 k11 d5 asymmetric', 'bf16', (12, 0)): 0.0104,
    ('conv snake 128>128 k11 d5 asymmetric', 'bf16', (0, 2)): 0.0117,
    ('conv snake 128>128 k11 d5 asymmetric', 'bf16', (0, 4)): 0.0117,
    ('conv snake 128>128 k11 d5 asymmetric', 'bf16', (16, 0)): 0.0106,
    ('conv snake 128>128 k11 d5 asymmetric', 'f16', (-22, 0)): 0.0090,
    ('conv snake 128>128 k11 d5 asymmetric', 'f16', (-18, 0)): 0.0075,
    ('conv snake 128>128 k11 d5 asymmetric', 'f16', (-14, 0)): 0.0112,
    ('conv snake 128>128 k11 d5 asymmetric', 'f16', (12, 0)): 0.0129,
    ('conv snake 128>128 k11 d5 asymmetric', 'f16', (0, 2)): 0.0139,
    ('conv snake 128>128 k11 d5 asymmetric', 'f16', (0, 4)): 0.0154,
    ('conv snake 128>128 k11 d5 asymmetric', 'f16', (13, 0)): 0.0126,
    ('resblock lrelu 128 k3 16-bit stream', 'bf16', (-22, 0)): 0.0097,
    ('resblock lrelu 128 k3 16-bit stream', 'bf16', (-18, 0)): 0.0097,
    ('resblock lrelu 128 k3 16-bit stream', 'bf16', (-14, 0)): 0.0097,
    ('resblock lrelu 128 k3 16-bit stream', 'bf16', (12, 0)): 0.0097,
    ('resblock lrelu 128 k3 16-bit stream', 'bf16', (16, 0)): 0.0097,
    ('resblock lrelu 128 k3 16-bit stream', 'f16', (-22, 0)): 0.0026,
    ('resblock lrelu 128 k3 16-bit stream', 'f16', (-18, 0)): 0.0031,
    ('resblock lrelu 128 k3 16-bit stream', 'f16', (-14, 0)): 0.0043,
    ('resblock lrelu 128 k3 16-bit stream', 'f16', (12, 0)): 0.0039,
    ('resblock mfma snake 32 k3 16-bit stream', 'bf16', (-22, 0)): 0.0171,
    ('resblock mfma snake 32 k3 16-bit stream', 'bf16', (-18, 0)): 0.0100,
    ('resblock mfma snake 32 k3 16-bit stream', 'bf16', (-14, 0)): 0.0182,
    ('resblock mfma snake 32 k3 16-bit stream', 'bf16', (12, 0)): 0.0186,
    ('resblock mfma snake 32 k3 16-bit stream', 'bf16', (0, 2)): 0.0195,
    ('resblock mfma snake 32 k3 16-bit stream', 'bf16', (0, 4)): 0.0355,
    ('resblock mfma snake 32 k3 16-bit stream', 'f16', (-22, 0)): 0.0189,
    ('resblock mfma snake 32 k3 16-bit stream', 'f16', (-18, 0)): 0.0141,
    ('resblock mfma snake 32 k3 16-bit stream', 'f16', (-14, 0)): 0.0098,
    ('resblock mfma snake 32 k3 16-bit stream', 'f16', (12, 0)): 0.0170,
    ('resblock mfma snake 32 k3 16-bit stream', 'f16', (0, 2)): 0.0206,
    ('resblock mfma snake 32 k3 16-bit stream', 'f16', (0, 4)): 0.0308,
    ('resblock mfma snake 128 k11 d5 stored', 'bf16', (-22, 0)): 0.0107,
    ('resblock mfma snake 128 k11 d5 stored', 'bf16', (-18, 0)): 0.0107,
    ('resblock mfma snake 128 k11 d5 stored', 'bf16', (-14, 0)): 0.0154,
    ('resblock mfma snake 128 k11 d5 stored', 'bf16', (12, 0)): 0.0159,
    ('resblock mfma snake 128 k11 d5 stored', 'bf16', (0, 2)): 0.0153,
    ('resblock mfma snake 128 k11 d5 stored', 'bf16', (0, 4)): 0.0165,
    ('resblock mfma snake 128 k11 d5 stored', 'f16', (-22, 0)): 0.0097,
    ('resblock mfma snake 128 k11 d5 stored', 'f16', (-18, 0)): 0.0066,
    ('resblock mfma snake 128 k11 d5 stored', 'f16', (-14, 0)): 0.0126,
    ('resblock mfma snake 128 k11 d5 stored', 'f16', (12, 0)): 0.0178,
    ('resblock mfma snake 128 k11 d5 stored', 'f16', (0, 2)): 0.0193,
    ('resblock mfma snake 128 k11 d5 stored', 'f16', (0, 4)): 0.0179,
    ('resblock valu snake 256 k3 16-bit stream', 'bf16', (-22, 0)): 0.0074,
    ('resblock valu snake 256 k3 16-bit stream', 'bf16', (-18, 0)): 0.0071,
    ('resblock valu snake 256 k3 16-bit stream', 'bf16', (-14, 0)): 0.0074,
    ('resblock valu snake 256 k3 16-bit stream', 'bf16', (12, 0)): 0.0049,
    ('resblock valu snake 256 k3 16-bit stream', 'bf16', (0, 2)): 0.0112,
    ('resblock valu snake 256 k3 16-bit stream', 'bf16', (0, 4)): 0.0079,
    ('resblock valu snake 256 k3 16-bit stream', 'bf16', (16, 0)): 0.0073,
    ('resblock valu snake 256 k3 16-bit stream', 'f16', (-22, 0)): 0.0078,
    ('resblock valu snake 256 k3 16-bit stream', 'f16', (-18, 0)): 0.0069,
    ('resblock valu snake 256 k3 16-bit stream', 'f16', (-14, 0)): 0.0061,
    ('resblock valu snake 256 k3 16-bit stream', 'f16', (12, 0)): 0.0052,
    ('resblock valu snake 256 k3 16-bit stream', 'f16', (0, 2)): 0.0104,
    ('resblock valu snake 256 k3 16-bit stream', 'f16', (0, 4)): 0.0189,
    ('wavenet layer cout2 384', 'bf16', (-22, 0)): 0.0028,
    ('wavenet layer cout2 384', 'bf16', (-18, 0)): 0.0056,
    ('wavenet layer cout2 384', 'bf16', (-14, 0)): 0.0057,
    ('wavenet layer cout2 384', 'bf16', (12, 0)): 0.1165,
    ('wavenet layer cout2 384', 'bf16', (16, 0)): 0.0862,
    ('wavenet layer cout2 384', 'f16', (-22, 0)): 0.0040,
    ('wavenet layer cout2 384', 'f16', (-18, 0)): 0.0026,
    ('wavenet layer cout2 384', 'f16', (-14, 0)): 0.0060,
    ('wavenet layer cout2 384', 'f16', (12, 0)): 0.4278,
    ('wavenet layer cout2 384', 'f16', (13, 0)): 0.4524,
    ('ffn 1536 post 300 rows', 'bf16', (-22, 0)): 0.0099,
    ('ffn 1536 post 300 rows', 'bf16', (-18, 0)): 0.0132,
    ('ffn 1536 post 300 rows', 'bf16', (-14, 0)): 0.0090,
    ('ffn 1536 post 300 rows', 'bf16', (12, 0)): 0.0191,
    ('ffn 1536 post 300 rows', 'bf16', (16, 0)): 0.0327,
    ('ffn 1536 post 300 rows', 'f16', (-22, 0)): 0.0100,
    ('ffn 1536 post 300 rows', 'f16', (-18, 0)): 0.0110,
    ('ffn 1536 post 300 rows', 'f16', (-14, 0)): 0.0093,
    ('ffn 1536 post 300 rows', 'f16', (12, 0)): 0.0513,
    ('ffn 1536 post 300 rows', 'f16', (16, 0)): 0.0336,
    ('attention gentle [129, 31, 33]', 'f16', (-22, 0)): 0.0483,
    ('attention gentle [129, 31, 33]', 'f16', (-18, 0)): 0.0225,
    ('attention gentle [129, 31, 33]', 'f16', (-14, 0)): 0.0225,
    ('attention gentle [129, 31, 33]', 'f16', (12, 0)): 0.0225,
    ('attention gentle [129, 31, 33]', 'f16', (13, 0)): 0.0225,
}
