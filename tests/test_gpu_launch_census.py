"""Which kernels one seeded trunk step launches, and how large the engine's workspace is, under the default environment and under
every group of switches in test_gpu_variants.ENGINE_VARIANTS -- compared EXACTLY with tests/golden/launch_census.json.

The step: a bf16 ResNet-50 trunk on 4 images of 128 x 128 (layer 1 runs at 32 pixels, inside the 28..60 window of the halo weight
gradient; layers 1-2 take the y3-free / Gram / row-streaming conv3 path; the stem takes the fused apply + pool; the eval forward
at 4 images splits K in layer 4), one training forward + backward and one eval forward, with the engine's per-launch profile on.
The census is {workspace_bytes, launches: {kernel symbol: count}}.

The test runs in the main suite process as `default`, and again inside every variant child of test_gpu_variants.py, where its
key is the variant's id.  That makes the variants non-vacuous: a switch name that is mistyped or no longer read leaves the child on
the default census, which is not what the fixture holds for it.  Visibility is promised per VARIANT, not per switch: a group of
switches must move the census as a whole; a single switch inside a group may leave it alone (RPE_NO_WALK_ALT only changes the
order in which a kernel walks its tiles).  Groups that only change the schedule are listed in SCHEDULE_ONLY with the reason.

A pull request that changes the launch plan on purpose re-records the fixture (python tests/test_gpu_launch_census.py on the GPU
box); the diff of the JSON then shows what moved."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from test_gpu_variants import ENGINE_VARIANTS

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "launch_census.json")
BATCH, SIDE, LATENT = 4, 128, 32

# variants whose census equals the default one, and why that is right
SCHEDULE_ONLY = {
    "RPE_NO_OVERLAP=1": "the same launches, all on the caller's stream (the test asserts that no second stream was created)",
    "RPE_SIDE_LOW_PRIO=1,RPE_TEST_STREAM_SKIP=3": "the same launches; only the second stream's priority and position in the process change",
}


def variant_id(env):
    """The key of the fixture: the variables of `env` whose names occur in ENGINE_VARIANTS, in the order the variants list them
    (the id pytest gives the variant's case); none of them set: 'default'."""
    names = [k for v in ENGINE_VARIANTS for k in v]
    return ",".join("%s=%s" % (k, env[k]) for k in names if k in env) or "default"


def census_step():
    """-> (census, features, gradient arena, second-stream candidates) of the seeded step"""
    import torch

    from rgb_proprioceptive_pose_estimator_amd import ops
    from rgb_proprioceptive_pose_estimator_amd._lib import lib
    from rgb_proprioceptive_pose_estimator_amd.engine import ResNet50Trunk
    from rgb_proprioceptive_pose_estimator_amd.params import ParamArena

    torch.manual_seed(1234)
    trunk = ResNet50Trunk(LATENT, compute_dtype=torch.bfloat16, depth=50).cuda().train()
    trunk.ensure_layout()
    arena = ParamArena(trunk)
    g = torch.Generator().manual_seed(99)
    img = torch.randn(BATCH, 3, SIDE, SIDE, generator=g).cuda()
    d_feat = (torch.randn(BATCH, ops.pad4(LATENT), generator=g) / BATCH).cuda()
    feat = torch.zeros(BATCH, ops.pad4(LATENT), device="cuda")
    feat_eval = torch.zeros_like(feat)
    plan = trunk.run(img, feat, True, pre_forward=lambda p: lib.rpe_resnet50_profile(p.handle, 1))
    plan.backward(d_feat, False)
    assert trunk.run(img, feat_eval, False) is plan
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    nbytes = lib.rpe_resnet50_profile_kernels(plan.handle, buf, len(buf))
    assert nbytes > 0
    launches = {}
    for line in buf.raw[:nbytes].decode().splitlines():
        name, cnt = line.split(";")[:2]
        launches[name] = launches.get(name, 0) + int(cnt)
    lib.rpe_resnet50_profile(plan.handle, 0)
    cand, conc = ctypes.c_int(), ctypes.c_int()
    lib.rpe_resnet50_side_stream_info(plan.handle, ctypes.byref(cand), ctypes.byref(conc))
    census = {"workspace_bytes": int(lib.rpe_resnet50_workspace_bytes(plan.handle)), "launches": dict(sorted(launches.items()))}
    return census, feat, arena.grad, cand.value


@pytest.mark.gpu
def test_launch_census():
    key = variant_id(os.environ)
    expected = json.load(open(FIXTURE))[key]
    census, _, _, candidates = census_step()
    print("census[%s] = %s, second-stream candidates %d" % (key, json.dumps(census), candidates))
    assert census == expected, "launch census of %r moved:\n got  %s\n want %s" % (key, json.dumps(census), json.dumps(expected))
    if "RPE_NO_OVERLAP" in os.environ:
        assert candidates == 0, candidates
    else:
        assert 1 <= candidates <= 4, candidates


def test_every_variant_is_visible_in_the_fixture():
    """the fixture alone: one entry per variant + default, and every variant outside SCHEDULE_ONLY differs from default"""
    fx = json.load(open(FIXTURE))
    ids = [variant_id(v) for v in ENGINE_VARIANTS]
    assert sorted(fx) == sorted(ids + ["default"])
    assert set(SCHEDULE_ONLY) <= set(ids)
    for i in ids:
        assert (fx[i] == fx["default"]) == (i in SCHEDULE_ONLY), i
    # the paths the variants switch off are in the default census
    names = list(fx["default"]["launches"])
    for part in ("wgrad_halo_kernel", "conv1x1_stream_fwd_kernel", "bn_apply_gram_kernel", "bn_gram_stats_kernel", "bn_apply_maxpool_kernel",
                 "nt_split_epilogue_kernel"):
        assert any(n.startswith(part) for n in names), part
    # nt_kernel<type, waves, BN, KCH, MODE, stages, ROLE, bn>: MODE 3 is the halo form; ROLE 0 the training forward, 1 the data gradient
    halo = {n.split(",")[6] for n in names if n.startswith("nt_kernel<") and n.split(",")[4] == "3"}
    assert {"0", "1"} <= halo, halo


def _record():
    """default and every variant as child processes, one after the other, each under its own time limit; stops at the first bad exit"""
    out = {}
    for env in [{}] + ENGINE_VARIANTS:
        child_env = dict(os.environ)
        child_env.update(env)
        r = subprocess.run(["timeout", "-k", "10", "180", sys.executable, os.path.abspath(__file__), "--child"], env=child_env,
                           cwd=os.path.dirname(HERE), capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("census child %r ended with status %d:\n%s%s" % (env, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
        out[variant_id(env)] = json.loads(r.stdout.strip().splitlines()[-1])
        print(variant_id(env), flush=True)
    with open(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    if "--child" in sys.argv:
        print(json.dumps(census_step()[0]))
    else:
        _record()
