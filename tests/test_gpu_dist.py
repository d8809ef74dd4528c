"""Two data-parallel ranks on ONE GPU over gloo (RCCL refuses two ranks per device): exercises the staged all-reduce that
runs under the backward and checks it against the one-shot reduction and against rank-local gradients."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from rgb_proprioceptive_pose_estimator_amd import models as M
    from rgb_proprioceptive_pose_estimator_amd.dist import GradSync, broadcast_parameters, init_from_env, stage_slices
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import synthetic_batch

    init_from_env("gloo")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    torch.manual_seed(rank)  # different init per rank: broadcast must fix it
    model = M.NaiveObjectStateEstimator("cube", [32], 50, 32, False, (9,), False, False, False, compute_dtype=torch.float32).cuda().train()
    model._materialize(dev)
    broadcast_parameters(model._arena.flat, list(model.buffers()))
    crit = M.PoseDistanceLoss("combined", 1.0, 0.5, 1e-4, "pose")
    b = synthetic_batch((2,), 100 + rank)

    def backward():
        model._arena.zero_grad()            # a fresh gradient per call (torch semantics would otherwise accumulate)
        crit(model(b["img"], None, b["x0bar"]), b["obj"]).backward()
        return model._arena.grad.clone()

    local = backward()                      # rank-local gradient, no reduction
    sync = GradSync(model._arena.grad, bucket_bytes=8 << 20).attach(model)
    sl = stage_slices(model)
    covered = sorted(v for v in sl.values() if v[1] > v[0])
    ok = covered[0][0] == 0 and covered[-1][1] == model._arena.numel and all(a[1] == c[0] for a, c in zip(covered, covered[1:]))
    staged = backward()
    sync.finish()
    staged = model._arena.grad.clone()      # after finish(): SUM over ranks, reduced stage by stage under the backward
    model._grad_sync = None
    oneshot = local.clone()
    dist.all_reduce(oneshot)                # reference: reduce the rank-local gradients in one go
    # wgrad uses fp32 atomics: two backward passes agree to ~1e-6 relative, not bitwise
    scale = oneshot.abs().max().item()
    err = (staged - oneshot).abs().max().item() / scale
    # model level: the reduced gradient == the SUM of the shard gradients as ONE process computes them, shard by shard, on the same
    # weights.  (BatchNorm statistics are per replica -- as under the reference's nn.DataParallel, models/naive.py:253 -- so the sum of
    # shard gradients is what data parallelism means for this net; the gradient of the CONCATENATED batch under whole-batch
    # statistics differs by design, and the engine has no eval-mode-BatchNorm backward to make the two coincide.)
    other = synthetic_batch((2,), 100 + (1 - rank))
    model._arena.zero_grad()
    crit(model(other["img"], None, other["x0bar"]), other["obj"]).backward()
    both = local + model._arena.grad
    err_model = (staged - both).abs().max().item() / scale
    # gradient accumulation under the staged reduction (torch semantics: a second backward() without zero_grad() ADDS): two backward passes
    # on the rank's batch, reduced stage by stage, must leave 2 x the reduced gradient
    model._grad_sync = sync
    model._arena.zero_grad()
    crit(model(b["img"], None, b["x0bar"]), b["obj"]).backward()
    sync.finish()
    crit(model(b["img"], None, b["x0bar"]), b["obj"]).backward()      # no zero_grad(): accumulates
    sync.finish()
    err_acc = (model._arena.grad - 2 * staged).abs().max().item() / scale
    model._grad_sync = None
    q.put((rank, ok, err, float((staged - local).abs().max().item() / scale), max(err_model, err_acc)))
    dist.destroy_process_group()


def test_staged_allreduce_two_ranks_one_gpu():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for rank, ok, err, moved, err_model in res:
        assert ok, "stage slices do not tile the arena"
        assert err < 1e-4, "staged all-reduce differs from the one-shot reduction: %g" % err
        assert moved > 1e-3, "gradients were not reduced (staged == local)"
        assert err_model < 1e-4, "reduced gradient differs from the single-process sum of the two shard gradients: %g" % err_model


def _rccl_worker(port, q):
    # a fresh process that has not touched the GPU yet: RCCL ("nccl" on ROCm) with ONE rank -- the communicator is created and
    # every bucket of the staged gradient reduction runs through ncclAllReduce on the device, which is what an N-GPU run
    # does per rank (no 8-GPU node is available to this test)
    os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RPE_DIST_FORCE_INIT="1")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch.distributed as dist
    from rgb_proprioceptive_pose_estimator_amd import models as M
    from rgb_proprioceptive_pose_estimator_amd.dist import GradSync, broadcast_parameters, init_from_env
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import synthetic_batch
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import train_step

    rank, world, local = init_from_env()          # backend chosen by dist.py: "nccl" when a GPU is visible
    assert dist.is_initialized() and dist.get_backend() == "nccl" and world == 1
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    torch.manual_seed(0)
    model = M.NaiveObjectStateEstimator("cube", [32], 50, 32, False, (9,), False, False, False, compute_dtype=torch.bfloat16).cuda().train()
    model._materialize(dev)
    dist.broadcast(model._arena.flat, 0)          # RCCL broadcast (what broadcast_parameters issues for world > 1)
    crit = M.PoseDistanceLoss("combined", 1.0, 0.5, 1e-4, "pose")
    criterion = {"obj_loss": crit, "val_loss": M.PoseDistanceLoss(mode="val")}
    opt = FusedAdam(model.parameters(), lr=1e-3)
    b = synthetic_batch((4,), 5)
    batch = (b["img"], None, b["x0bar"], b["x0"], None, b["obj"])
    crit(model(b["img"], None, b["x0bar"]), b["obj"]).backward()
    local_grad = model._arena.grad.clone()
    sync = GradSync(model._arena.grad, bucket_bytes=8 << 20, reduce_single=True).attach(model)
    n_calls = [0]
    orig = sync.reduce_range

    def counted(lo, hi):
        n_calls[0] += len(sync.buckets(lo, hi)) if hi > lo else 0
        return orig(lo, hi)

    sync.reduce_range = counted
    loss, _, _ = train_step(model, batch, criterion, opt, True, "train", sync)   # staged all-reduce under the backward, then Adam
    torch.cuda.synchronize()
    # a 1-rank SUM leaves the gradients as they are (up to fp32 atomic-order noise between two backward passes)
    err = ((model._arena.grad - local_grad).norm() / local_grad.norm()).item()
    q.put((dist.get_backend(), n_calls[0], err, bool(torch.isfinite(loss).item())))
    dist.destroy_process_group()


def test_rccl_backend_single_rank_staged_step():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_worker, args=(_free_port(), q))
    p.start()
    backend, calls, err, finite = q.get(timeout=300)
    p.join(timeout=120)
    assert p.exitcode == 0
    assert backend == "nccl" and calls >= 5 and finite
    assert err < 1e-4


def test_bench_two_ranks_sharing_one_gpu():
    """The driver's multi-GPU command line (`python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...`), rehearsed with two
    gloo ranks on the one GPU at a small batch: both ranks must run the same number of steps (the pre-conditioning loop is time-based,
    so rank 0 decides for all), rank 0 prints ONE JSON line with the whole-job throughput."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RPE_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
           str(_free_port()), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2", "--batch", "16", "--no-cpu-baseline", "--precondition-min", "1"]
    r = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["warmup"] == 2 and d["scaling"] == "weak"
    assert d["config"]["global_batch"] == 32 and d["config"]["parallelism"] == "dp2"
    assert d["value"] > 0 and abs(d["value"] - 32 / (d["ms_per_step"] * 1e-3)) < 0.01 * d["value"]


def test_bench_data_parallel_path_host_stays_ahead_of_the_device():
    """`bench.py --force-dist` (an RCCL world of one rank: the staged joins and bucketed all-reduce of an N-GPU run, on this one GPU) at
    128 images: the line carries the host's issue time per step measured on isolated steps, and the host must be comfortably ahead of
    the device -- a data-parallel rank whose host needs longer to ISSUE a step than the device needs to run it scales with the host."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--force-dist", "--full", "--steps", "6", "--warmup", "2", "--batch", "128", "--no-cpu-baseline", "--precondition-min", "1"]
    r = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["host_issue_ms_per_step"] < 8.0, d["host_issue_ms_per_step"]
    assert d["host_issue_ms_per_step"] < 0.7 * d["ms_per_step"], (d["host_issue_ms_per_step"], d["ms_per_step"])
