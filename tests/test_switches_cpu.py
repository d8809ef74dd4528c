"""The RPE_* environment switches, from the sources alone: every name the library (csrc/) or the Python package reads has a row in
INTEGRATION.md section 5 that says when it is read, and is either set by a group of tests/test_gpu_variants.py -- whose children
check which kernels they launch, tests/test_gpu_launch_census.py -- or excused here with a reason."""
import glob
import os
import re

from test_gpu_variants import ENGINE_VARIANTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgb-proprioceptive-pose-estimator_amd", "csrc")

# switches the Python package reads itself (ops.py at import, headops.py per call), and its other settings
PYTHON_SWITCHES = {"RPE_NO_LINEAR_ROWS", "RPE_NO_LINEAR_SPLITK", "RPE_STEM_UNFUSED", "RPE_NO_AUX_FUSE"}
PYTHON_SETTINGS = {"RPE_LIB_PATH", "RPE_DIST_BACKEND", "RPE_DIST_FORCE_INIT", "RPE_RESNET50_WEIGHTS", "RPE_BENCH_TOPK"}
# switches no group of ENGINE_VARIANTS sets, and why that is acceptable
NOT_IN_VARIANTS = {
    "RPE_NO_RELU_MASK": "fp32 engines take that path by themselves",
    "RPE_TN_WGS": "grid-size knob only (tools/ sweeps)",
    "RPE_TN_WGS_BIGM": "grid-size knob only (tools/ sweeps)",
    "RPE_WGRAD_HALO_WGS_NARROW": "grid-size knob only (tools/ sweeps)",
    "RPE_EW_UNR": "grid-size knob only (tools/sweep_ew.sh)",
    "RPE_EW_GRID": "grid-size knob only (tools/sweep_ew.sh)",
    "RPE_EW_NT": "load-policy knob of the same sweep (tools/sweep_ew.sh)",
    "RPE_NO_LINEAR_ROWS": "the tiled Linear launch it selects is what batches above 8 rows take by themselves",
}
WHEN = ("create", "process", "call", "create + process", "Python import", "Python call", "create + Python import", "process + Python call")


def _quoted(paths):
    """RPE_* names that stand alone in a string literal (ABI macros and enum names are never quoted on their own)"""
    names = set()
    for p in paths:
        names |= set(re.findall(r'"(RPE_[A-Z0-9_]+)"', open(p).read()))
    return names


def test_sources_agree():
    lib = _quoted(p for p in glob.glob(os.path.join(CSRC, "*")) if p.endswith((".hip", ".h")))
    py = _quoted(glob.glob(os.path.join(ROOT, "rgb-proprioceptive-pose-estimator_amd", "**", "*.py"), recursive=True) + [os.path.join(ROOT, "bench.py")])
    assert len(lib) == 36, sorted(lib)
    assert py == PYTHON_SWITCHES | PYTHON_SETTINGS, sorted(py ^ (PYTHON_SWITCHES | PYTHON_SETTINGS))
    # one row of INTEGRATION.md section 5 per variable, saying when it is read
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    documented = {}
    for line in doc[doc.index("## 5. Environment switches"):doc.index("## 6.")].splitlines():
        if not line.startswith("| `RPE_"):
            continue
        cells = [c.strip() for c in line.strip("|").split("|")]
        assert cells[1] in WHEN, line
        for n in re.findall(r"RPE_[A-Z0-9_]+", cells[0]):
            assert n not in documented, n
            documented[n] = cells[1]
    assert set(documented) == lib | py, sorted(set(documented) ^ (lib | py))
    assert all(("Python" in documented[n]) == (n in py) for n in documented)
    assert all(("create" in documented[n] or "process" in documented[n] or documented[n] == "call") == (n in lib) for n in documented)
    # every switch is exercised by a variant child, or excused here
    in_variants = {k for v in ENGINE_VARIANTS for k in v}
    switches = lib | PYTHON_SWITCHES
    assert in_variants <= switches, sorted(in_variants - switches)
    assert in_variants.isdisjoint(NOT_IN_VARIANTS)
    assert switches == in_variants | set(NOT_IN_VARIANTS), sorted(switches ^ (in_variants | set(NOT_IN_VARIANTS)))
