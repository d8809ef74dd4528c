"""The engine keeps a few switches that select an OLDER, still-needed code path (each is also what some configuration takes by itself:
fp32 engines have no packed ReLU mask, hooks on conv1 take the unfused stem backward, a missing slab workspace falls back to atomics,
one-stream execution is what a stream without a second queue gets).  Those paths must stay CORRECT.  The switches are listed in
INTEGRATION.md section 5 with the moment each is read: some when an engine is created, most once per process on first use, two at
every call, and four by the Python package (at import or per call) -- so every group gets one child process that runs golden train
steps under it.  The child also runs tests/test_gpu_launch_census.py, which holds the kernels it launches
against the variant's entry of tests/golden/launch_census.json: a group whose names are mistyped or no longer read fails there
instead of passing on the default path.  Children run one after the other (one GPU process at a time)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# schedule / fusion switches of the trunk engine: one golden train step per model family must still match the reference
ENGINE_VARIANTS = [
    {"RPE_NO_OVERLAP": "1"},        # everything on one stream
    {"RPE_SIDE_LOW_PRIO": "1", "RPE_TEST_STREAM_SKIP": "3"},   # round 2's low-priority second stream, created as the 4th stream of the process
    # projection-shortcut branch on the main stream; dense early-feature gradient + separate pool / BN backward passes for the
    # stem; conv3 backward through a materialised dy on the main stream
    {"RPE_NO_FWD_OVERLAP": "1", "RPE_STEM_UNFUSED": "1", "RPE_NO_BN_FOLD": "1"},
    # conv3 weight gradient from dy; fp32 atomics instead of slabs; the stem's BN apply and max pool as two passes (the eval path);
    # the 3x3 convs gather their activation operand per tap (the path
    # the fp32 engines and rows too wide for the halo patch take)
    {"RPE_NO_WGRAD_FOLD": "1", "RPE_WGRAD_ATOMIC": "1", "RPE_NO_HALO": "1", "RPE_NO_POOL_FUSE": "1"},
    # bn1's backward folded into conv1's gradients (y-form; measured slower in the step, off by default), every layer
    {"RPE_BN1_FOLD": "1", "RPE_BN1_FOLD_MAX": "512"},
    # the projection shortcut's BN as a pass of its own; folded weight gradient for layers 1-2 only; inference convs unsplit
    # (the golden case's eval / rollout outputs run at 2-4 images: the default takes the split-K kernels there)
    {"RPE_NO_SPLITK": "1", "RPE_NO_DS_FUSE": "1", "RPE_WGRAD_FOLD_MAX": "128", "RPE_NO_LINEAR_SPLITK": "1", "RPE_NO_DS_FOLD": "1"},
    # round 4: the round-3 bottleneck dataflow (y3 written, BN3 statistics from the conv epilogue, apply pass); the second stream unprobed
    {"RPE_NO_Y3FREE": "1", "RPE_NO_SIDE_PROBE": "1", "RPE_NO_AUX_FUSE": "1"},   # (+ the bn1 aux head as its own launch on a written a1)
    # the new forward (Gram statistics, fused conv3 epilogue) with y3 still written and the round-3 backward; Gram matrix as its own launch
    {"RPE_Y3_KEEP": "1", "RPE_NO_APPLY_GRAM": "1"},
    # y3-free with dz3^T a2 as the side product of the next block's fused conv1 data gradient (measured slower, off by default);
    # layer3 handled the same way as layers 1-2 where the shapes allow (Gram statistics for planes 256: the unfused Gram launch)
    {"RPE_T_FUSE": "1", "RPE_Y3FREE_MAX": "256"},
    # the y3-free conv3 forward as the tiled launch instead of the row-streaming kernel; every kernel walking its row tiles upwards;
    # the weight-gradient ring at two slots of 32 rows everywhere
    # ... and every 3x3 / stride-1 weight gradient in the gathered form (with the switches above: the first session's weight-gradient path)
    {"RPE_NO_STREAM1X1": "1", "RPE_NO_WALK_ALT": "1", "RPE_TN_RING": "1,2", "RPE_NO_WGRAD_HALO": "1"},
    # every 3x3 / stride-1 weight gradient in the halo form (maps down to 7 pixels, two workgroups per CU)
    {"RPE_WGRAD_HALO_MINW": "7", "RPE_WGRAD_HALO_WGS": "512"},
]


@pytest.mark.parametrize("env", ENGINE_VARIANTS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_engine_variant_parity(env):
    child_env = dict(os.environ)
    child_env.update(env)
    cmd = [sys.executable, "-m", "pytest", os.path.join(HERE, "test_gpu_models.py"), os.path.join(HERE, "test_gpu_launch_census.py"), "-q", "-x", "-p", "no:cacheprovider", "-k",
           "(test_model_fp32_matches_reference_and_oracle and tdo_v2) or (test_model_bf16_tracks_fp32_reference and no) or test_launch_census"]   # (fp32 golden step of a sequence model + the 16-bit path of the benchmarked model)
    r = subprocess.run(cmd, env=child_env, cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=900)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-1000:]
    assert r.returncode == 0, "variant %r failed:\n%s" % (env, tail)
    assert " passed" in r.stdout
