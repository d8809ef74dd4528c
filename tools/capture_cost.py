"""Diagnostic (GPU box): what the capture kernels cost for conv1's raw output (f0) of one frame and of a 100-frame episode, next to
the same tensor fetched through the engine's buffer with torch (`hooked_feature(0).permute(0, 3, 1, 2).float()`), each with and
without the copy to the host.  Wall-clock per call after warm-up; run it under `rocprofv3 --kernel-trace --stats -- python
tools/capture_cost.py` for the kernels' own time (feature_planes_kernel, minmax_init_kernel, feature_mosaic_kernel).

usage: python tools/capture_cost.py [bf16|f16|f32] [iterations]"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgb_proprioceptive_pose_estimator_amd import models as M  # noqa: E402
from rgb_proprioceptive_pose_estimator_amd import ops  # noqa: E402
from rgb_proprioceptive_pose_estimator_amd.util.data_utils import synthetic_batch  # noqa: E402
from rgb_proprioceptive_pose_estimator_amd.util.model_utils import capture_layer, layer_index_image  # noqa: E402

dtype = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[sys.argv[1] if len(sys.argv) > 1 else "bf16"]
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 10
torch.manual_seed(0)
model = M.NaiveObjectStateEstimator("cube", [64], 50, 64, False, (9,), False, False, True, compute_dtype=dtype).cuda().eval()
model.trunk.keep_stem_raw = True   # both forms then run ONE trunk forward per call (a conv1 hook's configuration)


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


for frames in (1, 100):
    img = synthetic_batch((frames,), 3)["img"]
    rows = torch.empty((frames, 64), dtype=torch.float32, device="cuda")

    def forward_only():
        with torch.no_grad():
            return model.trunk.run(img, rows, False)

    def torch_form():
        return forward_only().hooked_feature(0).permute(0, 3, 1, 2).float()

    def torch_form_minmax():
        t = torch_form()
        return t, t.amin(dim=(2, 3)), t.amax(dim=(2, 3))

    plan = forward_only()
    x = plan.hooked_feature(0)
    res = {
        "trunk forward alone": timed(forward_only),
        "capture_layer (device)": timed(lambda: capture_layer(model, "f0", img)),
        "capture_layer + .cpu()": timed(lambda: capture_layer(model, "f0", img).cpu()),
        "permute().float() (device)": timed(torch_form),
        "permute().float().cpu()": timed(lambda: torch_form().cpu()),
        "permute().float() + amin + amax (device)": timed(torch_form_minmax),
        "planes kernel alone": timed(lambda: ops.feature_planes(x)),
        "permute().float().contiguous() alone": timed(lambda: x.permute(0, 3, 1, 2).float().contiguous()),
    }
    if frames == 1:
        res["layer_index_image f0m (capture + mosaic + D2H)"] = timed(lambda: layer_index_image(model, "f0m", img))
    for k, v in res.items():
        print("f0 %s B=%-3d %-46s %8.3f ms" % (str(dtype).split(".")[-1], frames, k, v))
