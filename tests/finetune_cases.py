"""TEST INFRASTRUCTURE ONLY: the golden cases of the aligner's on-line fine-tuning (tests/golden/aligner/finetune.npz, made by
tests/golden/make_finetune_golden.py from the reference's own loop), their tolerance and the comparison with them, shared by the
CPU and the GPU tests."""
import os

import numpy as np

from ims_toucan_prosody_variance_amd import fixture_weights as fw
from tests import aligner_ref as ar
from tests import finetune_ref as fr

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aligner", "finetune.npz"))
N = int(G["n_cases"])
_REF = {}


def case(c):
    T = int(G[f"ft{c}_frames"])
    masks = np.unpackbits(G[f"ft{c}_masks"])[:5 * 5 * T * 512].reshape(5, 5, T, 512).astype(bool)
    return fw.aligner_spectrogram(int(G[f"ft{c}_seed"]), T), G[f"ft{c}_ids"], masks


def tol(c):
    """8 x the measured fp32-vs-fp64 distance of the reference's own fine-tuned logits, floor 1e-5 (the aligner's logit tolerance)."""
    return max(8.0 * float(G[f"ft{c}_sens"]), 1e-5)


def yardstick(c):
    """finetune_ref's float64 run of case c, computed once."""
    if c not in _REF:
        mel, ids, masks = case(c)
        _REF[c] = fr.fine_tune(fw.aligner_state_dict(), mel, ids, masks)
    return _REF[c]


def check_against_golden(c, logits, loss, norm, rm, rv):
    ref = G[f"ft{c}_logits"]
    top = float(np.abs(ref).max())
    errs = {"logits": float(np.abs(logits - ref).max()) / top,
            "loss": float(np.abs(loss - G[f"ft{c}_loss"]).max() / G[f"ft{c}_loss"].max()),
            "norm": float(np.abs(norm - G[f"ft{c}_norm"]).max() / G[f"ft{c}_norm"].max()),
            "running_mean": float(np.abs(rm - G[f"ft{c}_running_mean"]).max() / max(1.0, np.abs(G[f"ft{c}_running_mean"]).max())),
            "running_var": float(np.abs(rv - G[f"ft{c}_running_var"]).max() / max(1.0, np.abs(G[f"ft{c}_running_var"]).max()))}
    print(f"fine-tune case {c}: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()) + f" (bound {tol(c):.1e})")
    assert all(v <= tol(c) for v in errs.values()), errs
    ids, flags = G[f"ft{c}_ids"], G[f"ft{c}_flags"]
    dur = ar.postprocess(ar.mas(np.asarray(logits, dtype=np.float32)[:, ids], log64=True)[0], flags)
    assert np.array_equal(dur, G[f"ft{c}_dur"])
