"""Global-batch BatchNorm on the fused HIP tail across ranks.

Two ranks share the one GPU over gloo (plain subprocesses with the torchrun environment, 127.0.0.1): the SyncBatchNorm
box head trains on the HIP units -- no library convolution, no dist._SyncBatchNormFn -- and reproduces the global batch;
one DROW trunk block does the same.  A one-rank `nccl` group captures the same step as one hipGraph and replays it
without host synchronisation."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = {"type": "box_reg", "input_dim": 3, "target_dim": 3, "dropout": 0.0}

WORKER = textwrap.dedent('''
    import os, sys, json
    import numpy as np, torch
    import torch.distributed as tdist
    sys.path.insert(0, os.environ["POF_REPO"])
    sys.path.insert(0, os.path.join(os.environ["POF_REPO"], "planar_optical_flow_amd"))
    from planar_optical_flow_amd import dist as pd, ops
    from src.model.get_model import get_model
    from src.depracted.model.dr_spaam import DROW

    torch.cuda.set_device(0)
    tdist.init_process_group("gloo")
    rank, world = tdist.get_rank(), tdist.get_world_size()
    assert world == 2
    torch.manual_seed(7)
    model = get_model(json.loads(os.environ["POF_CFG"])).cuda()
    pd.broadcast_parameters(model)
    pd.convert_sync_batchnorm(model)
    model.train()
    torch.manual_seed(11)
    drow = DROW().cuda()
    pd.convert_sync_batchnorm(drow).train()

    # the route: neither a library convolution nor the module form of SyncBatchNorm may run
    def _refuse(name):
        def raiser(*a, **k):
            raise AssertionError(name + " was called: the unit left the HIP route")
        return raiser
    torch.nn.Conv1d.forward = _refuse("nn.Conv1d.forward")
    pd.SyncBatchNorm1d.forward = _refuse("SyncBatchNorm1d.forward")
    pd._SyncBatchNormFn.apply = _refuse("_SyncBatchNormFn.apply")
    calls = [0]
    _stats = ops.bn_sync_forward_stats
    def counted(*a, **k):
        calls[0] += 1
        return _stats(*a, **k)
    ops.bn_sync_forward_stats = counted

    rng = np.random.default_rng(3)
    X = torch.from_numpy(rng.normal(0, 0.3, (16, 64, 3))).float().cuda()
    Y = torch.from_numpy(rng.normal(0, 0.3, (16, 3))).float().cuda()
    lo, hi = pd.shard_range(16)
    assert hi - lo == 8
    optim = torch.optim.Adam(model.parameters(), lr=1e-3)
    red = pd.GradientAllReduce(model)
    out = {"losses": []}
    for step in range(3):
        optim.zero_grad(set_to_none=False)
        before = calls[0]
        pred = model(X[lo:hi])
        out["stats_calls_per_forward"] = calls[0] - before
        loss = model.loss_fn(pred, Y[lo:hi])
        loss.backward()
        red()
        if step == 0:
            out["grad"] = red.bucket[:-1].detach().cpu().clone()
            out["running"] = torch.cat([b.detach().reshape(-1).float().cpu() for n, b in model.named_buffers()
                                        if "running" in n])
        optim.step()
        t = torch.tensor([loss.item()], dtype=torch.float64)
        tdist.all_reduce(t)
        out["losses"].append(t.item() / world)

    # one DROW trunk block with pooling, 10 sequences split 5 + 5
    g = torch.Generator().manual_seed(5)
    xs = torch.randn(10, 1, 48, generator=g)
    gz = torch.randn(10, 128, 24, generator=g)
    x = xs[5 * rank:5 * rank + 5].cuda().requires_grad_(True)
    before = calls[0]
    z = DROW._run_block_train(x, drow.conv_block_1, True)
    out["drow_stats_calls"] = calls[0] - before
    z.backward(gz[5 * rank:5 * rank + 5].cuda())
    out["drow_z"], out["drow_dx"] = z.detach().cpu(), x.grad.cpu()
    out["drow_running"] = torch.cat([b.detach().reshape(-1).float().cpu() for n, b in drow.conv_block_1.named_buffers()
                                     if "running" in n])
    torch.cuda.synchronize()
    torch.save(out, os.path.join(os.environ["POF_OUT"], "rank%d.pt" % rank))
    tdist.destroy_process_group()
''')


def _run_two_ranks(script, out_dir):
    port = 31000 + (os.getpid() % 2000)
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), POF_REPO=REPO, POF_OUT=str(out_dir), POF_CFG=json.dumps(CFG),
                   OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    try:
        outs = [p.communicate(timeout=240) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, (o, e) in zip(procs, outs):
        assert p.returncode == 0, e[-3000:]


def _global_batch():
    import torch
    rng = np.random.default_rng(3)
    X = torch.from_numpy(rng.normal(0, 0.3, (16, 64, 3))).float()
    Y = torch.from_numpy(rng.normal(0, 0.3, (16, 3))).float()
    return X, Y


def _float64_reference():
    """First step of the global batch on the CPU in float64, stock BatchNorm: (gradients in parameter order, zeros where
    the loss does not reach; running statistics after the step; loss)."""
    import torch
    from src.model.get_model import get_model
    X, Y = _global_batch()
    torch.manual_seed(7)
    ref = get_model(CFG).double().train()
    loss = ref.loss_fn(ref(X.double()), Y.double())
    loss.backward()
    grad = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in ref.parameters()])
    running = torch.cat([b.detach().reshape(-1) for n, b in ref.named_buffers() if "running" in n])
    return grad, running, float(loss.detach())


def _one_gpu_losses():
    """The same three steps in ONE process on the global batch through the one-GPU HIP route (plain BatchNorm1d)."""
    import torch
    from src.model.get_model import get_model
    X, Y = _global_batch()
    X, Y = X.cuda(), Y.cuda()
    torch.manual_seed(7)
    model = get_model(CFG).cuda().train()
    optim = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    for _ in range(3):
        optim.zero_grad(set_to_none=False)
        loss = model.loss_fn(model(X), Y)
        loss.backward()
        optim.step()
        losses.append(loss.item())
    return losses


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_train_on_the_hip_sync_route(tmp_path):
    """8 + 8 samples on two ranks == the 16-sample global batch: first-step gradients and running statistics against
    float64 stock BatchNorm, three Adam losses against the one-GPU HIP route; six sync-stats exchanges per forward and
    no library convolution / _SyncBatchNormFn (patched to raise in the workers).  The same workers run DROW's
    conv_block_1 (pooled) on 5 + 5 sequences against the single-process block on all 10."""
    import torch
    sys.path.insert(0, os.path.join(REPO, "planar_optical_flow_amd"))
    script = tmp_path / "worker_sync_hip.py"
    script.write_text(WORKER)
    _run_two_ranks(script, tmp_path)        # a failed worker fails the test here: nothing else is started
    got = [torch.load(tmp_path / ("rank%d.pt" % r)) for r in range(2)]
    assert got[0]["stats_calls_per_forward"] == got[1]["stats_calls_per_forward"] == 6
    assert got[0]["drow_stats_calls"] == 3

    want_grad, want_running, want_loss = _float64_reference()
    # both ranks hold the same reduced bucket
    assert torch.equal(got[0]["grad"], got[1]["grad"])
    err = float((got[0]["grad"].double() - want_grad).abs().max()) / float(want_grad.abs().max())
    print("first-step gradient error, of the largest reference gradient: %.3e" % err)
    run_err = float((got[0]["running"].double() - want_running).abs().max())
    print("running statistics after step 1: max abs error %.3e" % run_err)
    one_gpu = _one_gpu_losses()
    print("losses two ranks %r\n       one GPU   %r\n       float64 first step %r" % (got[0]["losses"], one_gpu, want_loss))
    print("relative loss differences: %r" % [abs(a - b) / abs(b) for a, b in zip(got[0]["losses"], one_gpu)])
    assert err <= 1e-4
    for r in range(2):
        assert torch.allclose(got[r]["running"].double(), want_running, rtol=1e-5, atol=1e-6)
    # the bar of test_two_rank_train_mode_sync_batchnorm_matches_global_batch; measured on an MI355X: 5.7e-7
    np.testing.assert_allclose(got[0]["losses"], one_gpu, rtol=1e-5)

    # DROW conv_block_1: the single-process block (plain BatchNorm1d, the one-shot tail) on all 10 sequences
    from src.depracted.model.dr_spaam import DROW
    torch.manual_seed(11)
    drow = DROW().cuda().train()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(10, 1, 48, generator=g).cuda().requires_grad_(True)
    gz = torch.randn(10, 128, 24, generator=g).cuda()
    z = DROW._run_block_train(x, drow.conv_block_1, True)
    z.backward(gz)
    z2 = torch.cat([got[0]["drow_z"], got[1]["drow_z"]]).cuda()
    dx2 = torch.cat([got[0]["drow_dx"], got[1]["drow_dx"]]).cuda()
    want_run = torch.cat([b.detach().reshape(-1).float() for n, b in drow.conv_block_1.named_buffers() if "running" in n])
    dx_err, dx_scale = float((dx2 - x.grad).abs().max()), max(float(x.grad.abs().max()), 1.0)
    print("DROW block: z max abs diff %.3e, dx %.3e of scale" % (float((z2 - z).abs().max()), dx_err / dx_scale))
    assert torch.allclose(z2, z, rtol=1e-5, atol=2e-5)
    assert dx_err <= 1e-4 * dx_scale
    for r in range(2):
        assert torch.allclose(got[r]["drow_running"].cuda(), want_run, rtol=1e-5, atol=1e-6)


CAPTURE_WORKER = textwrap.dedent('''
    import os, sys, json
    import torch
    import torch.distributed as tdist
    sys.path.insert(0, os.environ["POF_REPO"])
    sys.path.insert(0, os.path.join(os.environ["POF_REPO"], "planar_optical_flow_amd"))
    from planar_optical_flow_amd import dist as pd
    from planar_optical_flow_amd.graph_step import GraphedTrainStep, make_capturable
    from src.model.get_model import get_model

    torch.cuda.set_device(0)
    tdist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    cfg = json.loads(os.environ["POF_CFG"])

    def _refuse(name):
        def raiser(*a, **k):
            raise AssertionError(name + " was called: the unit left the HIP route")
        return raiser
    _conv_forward, _conv_refuse = torch.nn.Conv1d.forward, _refuse("nn.Conv1d.forward")
    # on the device only: the float64 reference below is the stock model on the CPU
    torch.nn.Conv1d.forward = lambda self, x: _conv_refuse() if x.is_cuda else _conv_forward(self, x)
    pd.SyncBatchNorm1d.forward = _refuse("SyncBatchNorm1d.forward")
    pd._SyncBatchNormFn.apply = _refuse("_SyncBatchNormFn.apply")

    torch.manual_seed(6)
    gm = get_model(cfg).cuda()
    pd.convert_sync_batchnorm(gm).train()
    torch.manual_seed(6)
    em = get_model(cfg).cuda()                      # the eager twin
    pd.convert_sync_batchnorm(em).train()
    gopt = torch.optim.Adam(gm.parameters(), lr=1e-3, amsgrad=True)
    eopt = torch.optim.Adam(em.parameters(), lr=1e-3, amsgrad=True)
    make_capturable(gopt)
    gred = pd.GradientAllReduce(gm, always=True)
    ered = pd.GradientAllReduce(em, always=True)
    x = torch.randn(12, 64, 3, device="cuda")
    y = torch.randn(12, 3, device="cuda")
    gstep = GraphedTrainStep(gm, gopt, {"input": x, "target": y}, reducer=gred)
    assert gstep._fused_collective and len(gstep._graphs) == 1
    cpu_ref = get_model(cfg).double().train()

    def ref_grads(weights, xb, yb):
        with torch.no_grad():
            for p, w in zip(cpu_ref.parameters(), weights):
                p.copy_(w.double().cpu())
        cpu_ref.zero_grad(set_to_none=True)
        cpu_ref.loss_fn(cpu_ref(xb.double().cpu()), yb.double().cpu()).backward()
        return [p.grad for p in cpu_ref.parameters()]

    def grad_err(m, ref):
        rs = max(r.abs().max().item() for r in ref if r is not None)
        return max((p.grad.double().cpu() - r).abs().max().item() for p, r in zip(m.parameters(), ref)
                   if r is not None and p.grad is not None) / rs

    res = {"loss": [], "graph_grad": [], "eager_grad": []}
    for it in range(4):
        xb = torch.randn(12, 64, 3, device="cuda")
        yb = torch.randn(12, 3, device="cuda")
        g_w = [p.detach().clone() for p in gm.parameters()]
        e_w = [p.detach().clone() for p in em.parameters()]
        torch.cuda.set_sync_debug_mode("error")     # a replay, and the eager step on nccl, never wait for the device
        gl = gstep({"input": xb, "target": yb})
        eopt.zero_grad(set_to_none=False)
        el = em.loss_fn(em(xb), yb)
        el.backward()
        ered()
        eopt.step()
        torch.cuda.set_sync_debug_mode("default")
        res["loss"].append(abs(gl.item() - el.item()) / max(abs(el.item()), 1e-6))
        res["graph_grad"].append(grad_err(gm, ref_grads(g_w, xb, yb)))
        res["eager_grad"].append(grad_err(em, ref_grads(e_w, xb, yb)))
    tdist.destroy_process_group()
    print("RESULT " + json.dumps(res))
''')


@pytest.mark.gpu
def test_sync_route_captures_and_replays_on_one_rank_nccl(tmp_path):
    """The SyncBatchNorm box head on the HIP route in a GraphedTrainStep with the gradient all-reduce, one-rank `nccl`
    group: four replays (and the eager twin's steps) under sync debug mode "error"; losses <= 1e-5 relative from the
    eager twin, gradients <= 1e-4 of scale from the float64 CPU reference.  nn.Conv1d.forward raises from before the
    capture.  (Own process: the group must not leak into the other tests.)"""
    script = tmp_path / "worker_capture.py"
    script.write_text(CAPTURE_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(33000 + os.getpid() % 2000), POF_REPO=REPO,
               POF_CFG=json.dumps(CFG), HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
    print("captured vs eager: loss %r, gradients vs float64: captured %r eager %r"
          % (res["loss"], res["graph_grad"], res["eager_grad"]))
    assert max(res["loss"]) <= 1e-5
    assert max(res["graph_grad"]) <= 1e-4 and max(res["eager_grad"]) <= 1e-4
