"""The launch plan of a step that takes the compact shortcut gradients, pinned like tests/test_gpu_launch_census.py pins the small one,
and the engine-level equivalence of the two forms under every group of switches in test_gpu_variants.ENGINE_VARIANTS.

The step: a bf16 ResNet-50 trunk on 16 images of 256 x 256, one training forward + backward with the per-launch profile on -- the
smallest step at which the zero-filled shortcut gradients of layers 2 / 3 / 4 reach one workgroup per CU (1024 / 512 / 256), so that
all three entry blocks run rpe_conv1x1s2_dgrad_compact and a conv1 data gradient with a compact addend (",sub" in its symbol).  The
4-image step of tests/golden/launch_census.json stays below that and keeps its plan.

Per variant (the default environment in this process, every other one in a child process of its own):
- {workspace_bytes, launches: {kernel symbol: count}} == tests/golden/launch_census_compact.json[variant id], exactly;
- the same step with all-zero dense hook gradients on layers 1-3 (zero-filled shortcut gradients, nothing added) gives the same
  features and gradient tensors: bit for bit, except under RPE_WGRAD_ATOMIC=1, whose weight gradients are fp32 atomics and do not
  repeat bitwise from run to run -- there within the 16-bit path's 2e-2 of each tensor's largest element.

Re-record after a deliberate change of the plan: python tests/test_gpu_shortcut_census.py  (on the GPU box)."""
import json
import os
import subprocess
import sys

import pytest

from test_gpu_launch_census import variant_id
from test_gpu_variants import ENGINE_VARIANTS

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "launch_census_compact.json")
BATCH, SIDE = 16, 256
ATOMIC_BAR = 2e-2


def step_pair():
    """-> {census, zero_filled_sub: [default, hooked], exact, worst} of the default step and the hooked one"""
    import torch

    import test_gpu_shortcut_compact as sc

    feat_a, grads_a, forms_a, census = sc.engine_step(False, torch.bfloat16, BATCH, SIDE)
    feat_b, grads_b, forms_b, _ = sc.engine_step(True, torch.bfloat16, BATCH, SIDE)
    exact = sc.same_bits(feat_a, feat_b)
    worst = 0.0
    for (name, a), (_, c) in zip(grads_a, grads_b):
        if not (torch.isfinite(a).all() and torch.isfinite(c).all()):
            worst = float("inf")
        exact = exact and sc.same_bits(a, c)
        worst = max(worst, float((a - c).abs().max() / c.abs().max().clamp_min(1e-30)))
    return {"census": census, "forms": [list(forms_a), list(forms_b)], "exact": bool(exact), "worst": worst}


def check(res, env):
    key = variant_id(env)
    expected = json.load(open(FIXTURE))[key]
    print("compact census[%s]: forms %s exact %s worst %.3g" % (key, res["forms"], res["exact"], res["worst"]))
    assert res["census"] == expected, "launch census of %r moved:\n got  %s\n want %s" % (key, json.dumps(res["census"]), json.dumps(expected))
    # the hooked run: three zero-filled shortcut gradients, no compact addend; the default run: at least one entry block compact
    # (RPE_T_FUSE=1 keeps the blocks whose conv1 data gradient carries the T side product zero-filled)
    (zf_a, sub_a), (zf_b, sub_b) = res["forms"]
    assert (zf_b, sub_b) == (3, 0) and sub_a >= 1 and zf_a + sub_a == 3, res["forms"]
    if "RPE_WGRAD_ATOMIC" in env:
        assert res["worst"] < ATOMIC_BAR, res["worst"]
    else:
        assert res["exact"], "compact and zero-filled steps differ under %r (worst rel %.3g)" % (key, res["worst"])


def run_child(env):
    child_env = dict(os.environ)
    child_env.update(env)
    r = subprocess.run(["timeout", "-k", "10", "180", sys.executable, os.path.abspath(__file__), "--child"], env=child_env, cwd=os.path.dirname(HERE),
                       capture_output=True, text=True)
    assert r.returncode == 0, "child %r ended with status %d:\n%s%s" % (env, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_compact_census_default():
    check(step_pair(), {k: os.environ[k] for v in ENGINE_VARIANTS for k in v if k in os.environ})


@pytest.mark.gpu
@pytest.mark.parametrize("env", ENGINE_VARIANTS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_compact_census_variant(env):
    check(run_child(env), env)


def test_compact_fixture_holds_the_compact_plan():
    """the fixture alone: one entry per variant + default, each with the compact gradient's dense launches and ',sub' symbols"""
    fx = json.load(open(FIXTURE))
    assert sorted(fx) == sorted([variant_id(v) for v in ENGINE_VARIANTS] + ["default"])
    for key, c in fx.items():
        sub = sum(n for name, n in c["launches"].items() if name.endswith(",sub>"))
        assert sub == (1 if "RPE_T_FUSE" in key else 3), (key, sub)


def _record():
    out = {}
    for env in [{}] + ENGINE_VARIANTS:
        res = run_child(env)
        out[variant_id(env)] = res["census"]
        print(variant_id(env), res["forms"], res["exact"], "%.3g" % res["worst"], flush=True)
    with open(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    if "--child" in sys.argv:
        print(json.dumps(step_pair()))
    else:
        _record()
