"""The comparison of two renditions without a GPU: the float64 restatement (tests/compare_ref.py) against a plain double loop and
against values that can be checked by hand, how wide its decisions are on the cases the GPU tests compare on, the host half of
compare.py (the table, the refusals, the launch plan, ``finalise``), and that the header, the binding and the library declare the
same entries."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import build, capi, compare
from tests import compare_ref as cr

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL = [n for n, (ta, tb) in enumerate(cr.CASE_SIZES) if ta * tb <= 65 * 130]
DB = 10.0 / math.log(10.0)


@pytest.mark.parametrize("n", range(len(cr.CASE_SIZES)))
def test_every_decision_of_the_cases_is_wide(n):
    """The GPU tests ask for the restatement's path exactly: no cell of a case may decide by less than 1e-10 relative, (4096, 64)
    included.  The path's length is inside its bounds."""
    Ta, Tb = cr.CASE_SIZES[n]
    a, b = cr.cases()[n]
    assert a.shape == (Ta, 13) and b.shape == (Tb, 13) and a.dtype == b.dtype == np.float32
    s = cr.solved(n)
    print(f"case {Ta} x {Tb}: smallest relative gap {s['gap']:.3e}, path of {len(s['path'])}")
    assert s["gap"] >= cr.MIN_GAP
    assert max(Ta, Tb) <= len(s["path"]) <= Ta + Tb - 1
    assert tuple(s["path"][0]) == (0, 0) and tuple(s["path"][-1]) == (Ta - 1, Tb - 1)
    step = np.diff(s["path"], axis=0)
    assert set(map(tuple, step)) <= {(1, 1), (1, 0), (0, 1)}


@pytest.mark.parametrize("n", SMALL)
def test_restatement_agrees_with_a_double_loop(n):
    a, b = cr.cases()[n]
    cost, path = cr.dtw_naive(a, b)
    s = cr.solved(n)
    assert cost == s["cost"] and np.array_equal(path, s["path"])


def test_identical_sequences_give_cost_zero_and_the_diagonal():
    a = cr.cases()[3][0]
    s = cr.dtw(a, a)
    assert s["cost"] == 0.0 and np.array_equal(s["path"], np.stack([np.arange(64)] * 2, axis=1))
    sums = cr.path_sums(a, a, s["path"])
    r = compare.finalise(sums, len(s["path"]), with_f0=False)
    assert r == {"mcd_db": 0.0, "diag_share": 1.0}


def test_a_constant_offset_on_one_coefficient():
    """b = a + delta on coefficient 4: the diagonal costs |delta| per frame (to float32 rounding of a + delta) and every cell off it
    several times as much, so the path is the diagonal and mcd_db = (10 / ln 10) sqrt(2) |delta|."""
    a = cr.cases()[3][0].astype(np.float64)
    b = a.copy()
    delta = -0.75
    b[:, 4] += delta
    a, b = a.astype(np.float32), b.astype(np.float32)
    off = np.sqrt(cr.squared_distance(a, b))[~np.eye(64, dtype=bool)]
    assert off.min() > 2 * abs(delta)
    s = cr.dtw(a, b)
    assert np.array_equal(s["path"][:, 0], s["path"][:, 1])
    r = compare.finalise(cr.path_sums(a, b, s["path"]), len(s["path"]), with_f0=False)
    assert abs(r["mcd_db"] - DB * math.sqrt(2.0) * abs(delta)) <= 1e-6 * r["mcd_db"]
    assert abs(s["cost"] - 64 * abs(delta)) <= 1e-6 * s["cost"]


def test_one_frame_against_many_runs_along_the_row():
    a, b = cr.cases()[1]
    s = cr.solved(1)
    assert np.array_equal(s["path"], np.stack([np.zeros(7, dtype=np.int32), np.arange(7, dtype=np.int32)], axis=1))
    assert s["cost"] == float(np.sqrt(cr.squared_distance(a, b)).cumsum()[-1])
    assert len(cr.solved(0)["path"]) == 1


@pytest.mark.parametrize("shape", [(4, 4), (3, 6), (6, 3)])
def test_an_exact_tie_takes_the_diagonal_first(shape):
    """All-zero cepstra: every predecessor ties at 0.  Diagonal, then up, then left with strict < means: from the last cell the
    walk back takes the diagonal while both indices are positive, then runs along the border - so the path goes up or left FIRST
    (from (0, 0)) and ends on the diagonal."""
    Ta, Tb = shape
    z = np.zeros((max(shape), 13), dtype=np.float32)
    s = cr.dtw(z[:Ta], z[:Tb])
    n = min(Ta, Tb)
    tail = np.stack([np.arange(Ta - n, Ta), np.arange(Tb - n, Tb)], axis=1)
    head = np.stack([np.arange(Ta - n), np.zeros(Ta - n, dtype=int)], axis=1) if Ta > Tb else np.stack([np.zeros(Tb - n, dtype=int), np.arange(Tb - n)], axis=1)
    assert s["cost"] == 0.0 and s["gap"] == 0.0
    assert np.array_equal(s["path"], np.concatenate([head, tail]).astype(np.int32))
    assert np.array_equal(cr.dtw_naive(z[:Ta], z[:Tb])[1], s["path"])


def test_path_sums_by_hand():
    a = np.zeros((3, 13), dtype=np.float32)
    b = np.zeros((3, 13), dtype=np.float32)
    b[:, 0] = 2.0
    path = [(0, 0), (1, 1), (1, 2), (2, 2)]
    fa, fb = np.array([100.0, 0.0, 200.0], dtype=np.float32), np.array([100.0, 150.0, 150.0], dtype=np.float32)
    s = dict(zip(cr.SUM_COLUMNS, cr.path_sums(a, b, path, fa, fb)))
    assert s["mcd"] == pytest.approx(4 * math.sqrt(8.0), rel=1e-15) and s["diag"] == 1
    assert (s["vv"], s["vuv"], s["gross"]) == (2, 2, 1)  # voiced pairs (100, 100) and (200, 150); 50 > 0.2 * 150
    assert s["sq_hz"] == 2500.0 and s["sq_cents"] == pytest.approx((1200 * math.log2(200 / 150)) ** 2, rel=1e-15)
    assert s["x"] == pytest.approx(math.log(100) + math.log(200), rel=1e-15) and s["xy"] == pytest.approx(math.log(100) ** 2 + math.log(200) * math.log(150), rel=1e-15)
    none = cr.path_sums(a, b, path)
    assert none[0] == s["mcd"] and not none[2:].any()


def test_finalise_on_hand_made_sums():
    col = {c: k for k, c in enumerate(compare.SUM_COLUMNS)}
    assert compare.SUM_COLUMNS == cr.SUM_COLUMNS == capi.DTW_SUM_COLUMNS and compare.N_SUMS == len(col) == 12
    s = np.zeros(12)
    s[col["mcd"]], s[col["diag"]] = 30.0, 6.0
    x, y = np.log([100.0, 200.0, 400.0]), np.log([110.0, 190.0, 420.0])
    s[col["vv"]], s[col["sq_hz"]], s[col["sq_cents"]] = 3, 600.0, 30000.0
    s[col["x"]], s[col["y"]], s[col["xx"]], s[col["yy"]], s[col["xy"]] = x.sum(), y.sum(), (x * x).sum(), (y * y).sum(), (x * y).sum()
    s[col["gross"]], s[col["vuv"]] = 1, 2
    r = compare.finalise(s, 10)
    assert r["mcd_db"] == pytest.approx(DB * 3.0, rel=1e-15) and r["diag_share"] == pytest.approx(6 / 9)
    assert r["f0_rmse_hz"] == pytest.approx(math.sqrt(200.0)) and r["f0_rmse_cents"] == pytest.approx(100.0)
    assert r["f0_corr"] == pytest.approx(np.corrcoef(x, y)[0, 1], rel=1e-12)
    assert (r["gpe"], r["vde"], r["ffe"]) == (pytest.approx(1 / 3), 0.2, pytest.approx(0.3))
    assert set(compare.finalise(s, 10, with_f0=False)) == {"mcd_db", "diag_share"}
    # no point with both sides voiced: the F0 measures are NaN, the voicing error stays
    none = s.copy()
    none[col["vv"]:col["gross"] + 1] = 0
    r = compare.finalise(none, 10)
    assert all(math.isnan(r[k]) for k in ("f0_rmse_hz", "f0_rmse_cents", "f0_corr", "gpe")) and r["vde"] == 0.2 and r["ffe"] == 0.2
    # one such point, or a constant track on either side: no correlation
    one = s.copy()
    one[col["vv"]], one[col["x"]], one[col["xx"]], one[col["y"]], one[col["yy"]], one[col["xy"]] = 1, x[0], x[0] ** 2, y[0], y[0] ** 2, x[0] * y[0]
    r = compare.finalise(one, 10)
    assert math.isnan(r["f0_corr"]) and not math.isnan(r["f0_rmse_hz"])
    flat = s.copy()
    flat[col["x"]], flat[col["xx"]], flat[col["xy"]] = 3 * x[0], 3 * x[0] ** 2, x[0] * y.sum()
    assert math.isnan(compare.finalise(flat, 10)["f0_corr"])
    assert math.isnan(compare.finalise(s, 1)["diag_share"])
    for bad in (0, -3):
        with pytest.raises(ValueError):
            compare.finalise(s, bad)
    with pytest.raises(ValueError):
        compare.finalise(s[:11], 10)


def test_validate_pairs_refuses():
    compare.validate_pairs([1, compare.MAX_FRAMES], [compare.MAX_FRAMES, 1])
    compare.validate_pairs([], [])
    for fa, fb, words in (([3, 4], [3], "pairs"), ([3, 0], [3, 3], "pair 1, side a"), ([3], [-2], "pair 0, side b"),
                          ([3, 3, compare.MAX_FRAMES + 1], [3, 3, 3], "pair 2, side a"), ([3], [compare.MAX_FRAMES + 1], "pair 0, side b"),
                          ([2.5], [3], "pair 0, side a")):
        with pytest.raises(ValueError, match=words):
            compare.validate_pairs(fa, fb)


def test_dct_table_and_constants():
    t = compare.dct_table(13)
    assert t.dtype == np.float64 and t.shape == (13, 80) and np.array_equal(t, cr.dct_table(13))
    k, m = 5, 17
    assert t[k - 1, m] == pytest.approx(math.sqrt(2 / 80) * math.log(10) * math.cos(math.pi * k * (m + 0.5) / 80), rel=1e-14)
    # the rows of a DCT-II are orthogonal, and c0 (the constant row) is left out: a flat log-mel has no cepstrum
    g = t @ t.T / math.log(10) ** 2
    assert np.allclose(g, np.eye(13), atol=1e-12) and np.abs(t.sum(axis=1)).max() < 1e-12
    assert compare.dct_table(32).shape == (32, 80) and compare.dct_table(1).shape == (1, 80)
    for bad in (0, 33, 2.5, True):
        with pytest.raises(ValueError):
            compare.dct_table(bad)
    assert compare.MAX_FRAMES == capi.DTW_MAX_FRAMES == 4096 and compare.MAX_SCRATCH_BYTES == 1 << 30
    # the restatement's correctly rounded cepstra of a flat log-mel are zero to rounding
    assert np.abs(cr.cepstra(np.full((2, 80), -3.5, dtype=np.float32))).max() < 1e-6


def test_back_pointer_bytes_and_launch_plan():
    assert compare.bp_bytes(1, 1) == 4 and compare.bp_bytes(5, 16) == 20 and compare.bp_bytes(5, 17) == 40
    assert compare.bp_bytes(4096, 4096) == 4 << 20
    sizes = [compare.bp_bytes(ta, tb) for ta, tb in cr.CASE_SIZES]
    assert min(sizes) <= compare.LDS_BP_BYTES < max(sizes)  # the cases lie on both sides of the LDS form's limit
    fa, fb = [ta for ta, _ in cr.CASE_SIZES], [tb for _, tb in cr.CASE_SIZES]
    assert compare.plan_launches(fa, fb) == [(0, 12)] and compare.plan_launches([], []) == []
    assert compare.plan_launches(fa, fb, max_scratch_bytes=1) == [(0, 8), (8, 12)]  # only the largest, pair 7, uses the scratch buffer
    assert compare.plan_launches(fa, fb, force_scratch=True, max_scratch_bytes=sizes[5] + sizes[6]) == [(0, 6), (6, 7), (7, 8), (8, 12)]
    plans = compare.plan_launches(fa, fb, force_scratch=True, max_scratch_bytes=1)
    assert plans == [(p, p + 1) for p in range(12)]  # a pair larger than the bound still gets its launch
    many = compare.plan_launches([4096] * 600, [4096] * 600)
    assert many == [(0, 256), (256, 512), (512, 600)]


def test_compare_header_binding_and_library_agree():
    """include/toucan_compare.h, capi.COMPARE_PROTOTYPES and the symbols libtoucan_hip.so exports are the same set, disjoint from
    every other table, with the argument counts, the constants and the struct the binding mirrors."""
    root = os.path.dirname(HERE)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "toucan_compare.h"), encoding="utf-8").read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(tts_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.COMPARE_PROTOTYPES) == ["tts_dtw", "tts_dtw_max_frames", "tts_dtw_path_sums", "tts_mel_cepstra"]
    tables = [getattr(capi, n) for n in dir(capi) if n.endswith("PROTOTYPES") and n != "COMPARE_PROTOTYPES"]
    assert len(tables) >= 9 and not any(set(declared) & set(t) for t in tables)
    macros = {k: int(v) for k, v in re.findall(r"#define\s+(TTS_[A-Z0-9_]+)\s+(\d+)", text)}
    assert {k: v for k, v in macros.items() if not k.startswith("TTS_DTW_SUM_")} == {
        "TTS_COMPARE_MELS": capi.COMPARE_MELS, "TTS_COMPARE_MAX_CEP": capi.COMPARE_MAX_CEP, "TTS_DTW_MAX_FRAMES": capi.DTW_MAX_FRAMES,
        "TTS_DTW_LDS_BP_BYTES": capi.DTW_LDS_BP_BYTES, "TTS_DTW_N_SUMS": capi.DTW_N_SUMS}
    assert {k[len("TTS_DTW_SUM_"):].lower(): v for k, v in macros.items() if k.startswith("TTS_DTW_SUM_")} == \
        {c: k for k, c in enumerate(capi.DTW_SUM_COLUMNS)}
    names = re.findall(r"\bint\s+(tts_[a-z0-9_]+)\s*\(", text)
    assert sorted(names) == declared
    for arg_list, name in zip(re.findall(r"\bint\s+tts_[a-z0-9_]+\s*\((.*?)\)\s*;", text, flags=re.S), names):
        n_args = 0 if arg_list.strip() == "void" else len(arg_list.split(","))
        assert n_args == len(capi.COMPARE_PROTOTYPES[name][1]), name
    fields = re.search(r"typedef struct TtsDtwPair \{(.*?)\}", text, flags=re.S).group(1)
    assert [f.strip() for decl in fields.split(";") if decl.strip() for f in decl.strip().split(" ", 1)[1].split(",")] == \
        [n for n, _ in capi.TtsDtwPair._fields_]
    assert ctypes.sizeof(capi.TtsDtwPair) == 32
    assert "compare.hip" in build.SOURCES
    build.build()
    handle = capi.lib()
    assert isinstance(handle, ctypes.CDLL)
    for n in declared:
        assert hasattr(handle, n) and getattr(handle, n).argtypes == capi.COMPARE_PROTOTYPES[n][1], n
    assert handle.tts_abi_version() == 15 and handle.tts_dtw_max_frames() == compare.MAX_FRAMES
