"""The environment switches and the kernels' conditional compilation are closed sets: a switch that selects between two forms
which pass the same tests and measure the same is deleted, not kept (DESIGN.md section 5 records what was tried)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ims-toucan-prosody-variance_amd")

# user-facing variables, the four switches the GPU tests flip, and the residual step's stagger (bench.py's own TOUCAN_BENCH_* are read by bench.py only)
SWITCHES = {
    "TOUCAN_PRECISION", "TOUCAN_MODELS_DIR", "TOUCAN_PY_SEQUENCER", "TOUCAN_HIP_LIB",
    "TOUCAN_NO_SPLIT_K", "TOUCAN_NO_SPLIT_K16", "TOUCAN_GEMM_ROWS_BF16", "TOUCAN_SNAKE_VALU",
    "TOUCAN_RB_STAGGER",  # the one tuning switch left: its removal changes device code and waits for a measured comparison
}


def _sources(*exts):
    return [p for e in exts for p in glob.glob(os.path.join(PKG, "**", "*." + e), recursive=True)]


def test_environment_switches_are_the_closed_list_and_documented():
    found = set()
    for path in _sources("py", "hip", "h"):
        found |= set(re.findall(r"TOUCAN_[A-Z0-9_]+", open(path).read()))
    assert found == SWITCHES
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    table = set(re.findall(r"^\| `(TOUCAN_[A-Z0-9_]+)", doc, re.M))
    assert SWITCHES <= table


def test_kernel_sources_have_no_conditional_compilation():
    paths = glob.glob(os.path.join(PKG, "csrc", "*"))
    assert len(paths) >= 17
    for path in paths:
        hits = re.findall(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif|else|endif)\b.*$", open(path).read(), re.M)
        assert not hits, f"{os.path.basename(path)}: {hits}"
