"""The bits of the prosody control entries on the kernel inputs of tests/test_gpu_prosody_scales.py and tests/test_gpu_prosody_curves.py
(seeds 23 and 29), for comparing two builds of the library (run on the MI355X box):

    python tools/prosody_bits.py OUT_A                      # this tree
    python tools/prosody_bits.py OUT_B --root <other tree>  # a built checkout of another commit
    python tools/prosody_bits.py --compare OUT_A OUT_B

Every mode of every entry: the scalar entry with all ones and with each utterance's scales on that utterance alone, the _v entry
with NULL and with SCALES, the _c entry with the constant, the neutral and the mixed table, each with and without scales, and
tts_prosody_stats after each.  Pitch, energy, durations and statistics go to one .npz per seed; --compare holds them against each
other as int32 bit patterns (NaN payloads included) and exits 1 on a difference."""
import argparse
import os
import sys


def dump(root, out):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import ims_toucan_prosody_variance_amd  # noqa: F401
    from ims_toucan_prosody_variance_amd import capi, engine
    from ims_toucan_prosody_variance_amd.ragged import Ragged
    from tests import prosody_curves_ref as cref, prosody_ref as ref, test_gpu_prosody_curves as tc

    dev = "cuda:0"
    lengths, scales = tc.LENGTHS, np.float32(tc.SCALES)
    R = sum(lengths)
    ops, rag = engine.Ops(dev), Ragged(lengths, dev)
    tables = {"constant": cref.constant(lengths, tc.CONSTS), "neutral": cref.neutral(R), "mixed": tc._mixed()[0]}
    to = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    os.makedirs(out, exist_ok=True)
    for seed in (23, 29):  # the kernel_batch fixtures of the two test modules
        rng = np.random.default_rng(seed)
        text = np.zeros((R, 62), dtype=np.float32)
        text[:, ref.F_VOICED] = rng.random(R) < 0.6
        text[:, ref.F_PHONEME] = rng.random(R) < 0.8
        text[:, ref.F_WORD_BOUNDARY] = rng.random(R) < 0.15
        text[:, ref.F_SILENCE] = rng.random(R) < 0.2
        text[0, ref.F_VOICED] = 1
        b = sum(lengths[:tc.UNVOICED])
        text[b:b + lengths[tc.UNVOICED], ref.F_VOICED] = 0
        raw = dict(text=text, pitch=(0.3 + 0.5 * rng.standard_normal(R)).astype(np.float32),
                   energy=(0.5 + 0.4 * rng.standard_normal(R)).astype(np.float32), dur=rng.integers(0, 13, R).astype(np.int32))
        got = {}

        def run(name, call, sl=slice(None), r=rag):
            t, p, e, d = (to(raw[k][sl].copy()) for k in ("text", "pitch", "energy", "dur"))
            call(t, p, e, d, r)
            stats = ops.prosody_stats(p, e, d, r, torch.full((r.n_seq, capi.PROSODY_STATS), -7.0, device=dev))
            for k, v in (("pitch", p), ("energy", e), ("dur", d), ("stats", stats)):
                got[f"{name}.{k}"] = v.cpu().numpy()

        run("scalar_ones", lambda t, p, e, d, r: ops.prosody_control(t, p, e, d, r, 1.0, 1.0, 1.0, 1.0))
        for u, (b0, n) in enumerate(zip(rag.begins, rag.lengths)):
            run(f"scalar_alone{u}", lambda t, p, e, d, r: ops.prosody_control(t, p, e, d, r, *tc.SCALES[u]), slice(b0, b0 + n), Ragged([n], dev))
        run("v_null", lambda t, p, e, d, r: ops.prosody_control_v(t, p, e, d, r, None))
        run("v_scales", lambda t, p, e, d, r: ops.prosody_control_v(t, p, e, d, r, to(scales)))
        for name, table in tables.items():
            for tag, s in (("", None), ("_scales", scales)):
                run(f"c_{name}{tag}", lambda t, p, e, d, r: ops.prosody_control_c(t, p, e, d, r, to(s), to(table)))
        torch.cuda.synchronize()
        np.savez(os.path.join(out, f"seed{seed}.npz"), **got)
        print(f"seed {seed}: {len(got)} arrays -> {out}")


def compare(a, b):
    import numpy as np
    ok = True
    for seed in (23, 29):
        x, y = (np.load(os.path.join(d, f"seed{seed}.npz")) for d in (a, b))
        assert sorted(x.files) == sorted(y.files) and len(x.files) == 4 * 13, x.files
        for k in x.files:
            same = x[k].shape == y[k].shape and np.array_equal(x[k].view(np.int32), y[k].view(np.int32))
            ok &= same
            print(f"seed {seed} {k}: shape {x[k].shape} {x[k].dtype}, NaN {int(np.isnan(x[k]).sum()) if x[k].dtype.kind == 'f' else 0}, bits equal: {same}")
    print("all equal:", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="+")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the built tree whose library runs")
    ap.add_argument("--compare", action="store_true")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.out))
    dump(os.path.abspath(args.root), args.out[0])
