"""GPU: the real HIP-backed module under DistributedDataParallel with TWO processes sharing the one visible GPU
(backend gloo, CUDA tensors) -- exercises exactly the wiring bench.py uses at N>1 (frozen unused parameters, static
reducer, custom autograd Functions feeding DDP's bucket hooks), which cannot be run over RCCL on a 1-GPU box."""
import os

import pytest
import torch
import torch.distributed as dist

from mp_util import free_port, run_bounded, spawn_with_retry

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from fiber_amd import lib, ops, parallel
    from fiber_amd.config import make_config
    from fiber_amd.modules import FIBERTransformerSS, fiber_utils
    from oracle import cases, detgen
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    parallel.init_distributed("gloo")
    lib.load()
    torch.manual_seed(0)                      # same initial weights on both ranks (DDP also broadcasts rank 0's)
    ops.manual_seed(rank)
    model = FIBERTransformerSS(make_config(**cases.TINY, learning_rate=1e-3, warmup_steps=0, max_steps=100))
    for n, p in model.named_parameters():
        if "alpha_" in n:
            p.data.fill_(0.5)
    parallel.freeze_unused(model, model.unused_parameter_names())
    model.to(dev).train()
    fiber_utils.set_task(model)
    (opt,), _ = model.configure_optimizers()
    net = parallel.wrap_ddp(model, dev)
    assert isinstance(net, torch.nn.parallel.DistributedDataParallel)
    b = detgen.synth_batch(4, 96, 12, 1000, seed=20 + rank, min_len=6)      # different shard per rank
    bd = {k: (v.to(dev) if isinstance(v, torch.Tensor) else [t.to(dev) for t in v] if isinstance(v, list) and isinstance(v[0], torch.Tensor) else v)
          for k, v in b.items()}
    bd["itm_labels_override"] = bd["itm_labels"]
    losses = []
    for _ in range(3):
        out_d = net(bd)
        loss = sum(v for k, v in out_d.items() if "loss" in k)
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        losses.append(loss.item())
    flat = torch.cat([p.detach().float().flatten() for p in model.parameters()]).cpu()
    gathered = [torch.zeros_like(flat) for _ in range(world)]
    dist.all_gather(gathered, flat)
    if rank == 0:
        torch.save({"same": bool(torch.equal(gathered[0], gathered[1])), "losses": losses,
                    "finite": bool(torch.isfinite(flat).all())}, out)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_ddp_on_one_gpu(tmp_path):
    assert torch.cuda.is_available()
    out = str(tmp_path / "r0.pt")
    spawn_with_retry(_worker, lambda port: (2, port, out), nprocs=2, deadline_s=150)
    res = torch.load(out)
    assert res["finite"] and all(l == l for l in res["losses"])
    assert res["same"], "parameters diverged across DDP ranks (gradient all-reduce / frozen-parameter wiring is wrong)"


def _worker_no_sync(rank, world, port, out):
    """Gradient accumulation on the REAL module (run.py:46,63 `accumulate_grad_batches`): micro-batch 0 under no_sync(),
    micro-batch 1 synchronising -- the all-reduced gradient must equal the rank-mean of the locally accumulated gradients of
    an un-wrapped copy of the module (custom autograd Functions + bucket views + accumulation into existing .grad)."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import copy
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from fiber_amd import lib, parallel
    from fiber_amd.config import make_config
    from fiber_amd.modules import FIBERTransformerSS, fiber_utils
    from oracle import cases, detgen
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    parallel.init_distributed("gloo")
    lib.load()
    torch.manual_seed(0)
    model = FIBERTransformerSS(make_config(**cases.TINY))
    for n, p in model.named_parameters():
        if "alpha_" in n:
            p.data.fill_(0.5)
    parallel.freeze_unused(model, model.unused_parameter_names())
    model.to(dev).eval()                                   # no dropout / DropPath: both copies compute the same function
    fiber_utils.set_task(model)
    local = copy.deepcopy(model)
    fiber_utils.set_task(local)
    net = parallel.wrap_ddp(model, dev, bf16_grads=False)

    def batch(seed):
        b = detgen.synth_batch(4, 96, 12, 1000, seed=seed, min_len=6)
        bd = {k: (v.to(dev) if isinstance(v, torch.Tensor) else [t.to(dev) for t in v] if isinstance(v, list) and isinstance(v[0], torch.Tensor) else v)
              for k, v in b.items()}
        bd["itm_labels_override"] = bd["itm_labels"]
        return bd
    micro = [batch(40 + 2 * rank), batch(41 + 2 * rank)]
    loss_of = lambda o: sum(v for k, v in o.items() if "loss" in k) / 2
    with net.no_sync():
        loss_of(net(micro[0])).backward()
    loss_of(net(micro[1])).backward()
    for mb in micro:
        loss_of(local(mb)).backward()
    worst, worst_name, errs = 0.0, None, []
    for (n, p), (_, q) in zip(model.named_parameters(), local.named_parameters()):
        if p.grad is None:
            assert q.grad is None, n
            continue
        ref = q.grad.detach().float().cpu()
        dist.all_reduce(ref)
        ref /= world
        got = p.grad.detach().float().cpu()
        # (key biases of softmax attention have mathematically ZERO gradients -- what the kernels produce for them is rounding noise of
        # the order 1e-6 whose value depends on the summation order, hence an absolute floor next to the relative measure)
        err = float((got - ref).norm() / max(float(ref.norm()), 1e-4))
        errs.append((round(err, 5), n, round(float(ref.norm()), 6)))
        if err > worst:
            worst, worst_name = err, n
    if rank == 0:
        torch.save({"worst": worst, "param": worst_name, "top": sorted(errs, reverse=True)[:8]}, out)
    dist.barrier()
    dist.destroy_process_group()


def test_no_sync_gradient_accumulation_real_module(tmp_path):
    assert torch.cuda.is_available()
    out = str(tmp_path / "r0.pt")
    spawn_with_retry(_worker_no_sync, lambda port: (2, port, out), nprocs=2, deadline_s=150)
    res = torch.load(out)
    assert res["worst"] < 1e-3, res          # identical kernels on identical inputs; only the fp32 summation order differs


def test_bench_contract_two_ranks_one_gpu():
    """bench.py exactly as the driver launches it at N > 1 (torch.distributed.run, one process per rank), with the backend
    switched to gloo so that two ranks can share the one visible GPU: rank 0 must print ONE JSON line with the contract keys,
    n_gpus = 2 and a whole-job value; with --full also the exposed all-reduce time, the forward-only and dominant-kernel timings."""
    import json
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    port = free_port()
    env = dict(os.environ, FIBER_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "8",
           "--full"]
    res = run_bounded(cmd, 240, cwd=root, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["warmup"] == 1 and d["scaling"] == "weak" and d["higher_is_better"] is True
    assert d["config"]["global_batch"] == 16 and d["config"]["parallelism"] == "dp2"
    assert abs(d["value"] - 16 / (d["ms_per_step"] * 1e-3)) < 0.05 * d["value"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in d["roofline"], k
    assert d["step_ms"]["allreduce_exposed"] is not None and d["fwd_ms_per_image"] > 0, d
    assert d["roofline"]["dominant_kernel"]["us"] > 0, d["roofline"]


def test_bench_self_spawns_two_ranks_one_gpu():
    """`python bench.py --gpus 2` with NO external launcher: bench.py re-executes itself under torch.distributed.run, the two
    ranks share the one visible GPU over gloo, and rank 0 prints the contract line with n_gpus = 2 and the process-group size."""
    import json
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["FIBER_DIST_BACKEND"] = "gloo"
    res = run_bounded([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "8",
                       "--no-extras"], 240, cwd=root, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["rccl_ranks"] == 2 and d["config"]["global_batch"] == 16
    assert len(d["step_ms"]["per_rank_mean"]) == 2


def test_bench_counts_the_launches_of_a_step_in_a_child_process():
    """`extra.launches_per_step` of the --full bench line: tools/probes/launch_count.py (torch.profiler, device activity) in a child under a deadline.
    Round 6 counts 1493 kernels + 12 copy commands per steady-state step, 1292 of the kernels from libfiber_hip.so (the review's bar: <= 1700)."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    d = bench.launches_per_step(8, budget_s=200.0)
    assert "error" not in d, d
    assert 1000 < d["kernels"] + d["copy_or_fill_commands"] <= 1700, d
    assert d["of_which_fiber_hip"] > 0.8 * d["kernels"], d


def test_bench_dumps_the_outputs_of_its_last_timed_step(tmp_path):
    """`bench.py --dump-outputs DIR`: after the timed steps the loss, the forward's outputs (a seeded sample of the MLM logits) and the
    updated parameters of the LAST timed step as float arrays, at most 64 MB; the line reports the timed steps it was asked for.
    Without --full the run measures nothing beyond the headline: no forward-only, dominant-kernel, batch-sweep or CPU timings."""
    import json
    import sys

    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    res = run_bounded([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "8",
                       "--dump-outputs", str(tmp_path / "out")], 240, cwd=root, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert not {"fwd_ms_per_image", "extra", "cpu_baseline"} & set(d) and "dominant_kernel" not in d["roofline"], sorted(d)
    got = {n[:-4]: np.load(tmp_path / "out" / n) for n in os.listdir(tmp_path / "out")}
    for k in ("loss", "mlm_loss", "itm_loss", "mlm_logits_sample", "itm_logits", "itm_labels", "param_norms", "param_sample"):
        assert k in got, (k, sorted(got))
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in got.values()), sorted(got)
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["itm_logits"].shape == (8 * 2,) and got["mlm_logits_sample"].shape == (1 << 20,)
    assert abs(got["loss"][0] - d["loss"]) < 1e-3 and abs(got["loss"][0] - got["mlm_loss"][0] - got["itm_loss"][0]) < 1e-3
