"""One-rank RCCL smoke (run on a GPU box): the flat gradient bucket all-reduced on device tensors, the
SyncBatchNorm forward / backward collectives and a plain all-reduce through backend "nccl" (= RCCL on ROCm)."""
import os
import sys

import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "planar_optical_flow_amd"))
from planar_optical_flow_amd import dist as pd          # noqa: E402
from src.model.get_model import get_model               # noqa: E402

os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
os.environ.setdefault("MASTER_PORT", "29533")
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
assert dist.get_backend() == "nccl" and dist.get_world_size() == 1
cfg = {"type": "box_reg", "input_dim": 3, "target_dim": 3, "dropout": 0.0}
torch.manual_seed(5)
ref = get_model(cfg).cuda().train()
torch.manual_seed(5)
model = get_model(cfg).cuda()
pd.convert_sync_batchnorm(model).train()
x = torch.randn(12, 64, 3, device="cuda")
y = torch.randn(12, 3, device="cuda")
model.loss_fn(model(x), y).backward()
ref.loss_fn(ref(x), y).backward()
red = pd.GradientAllReduce(model)
before = {i: p.grad.clone() for i, p in enumerate(red.params) if p.grad is not None}
red(force=True)                                   # ncclAllReduce on the device bucket, one rank
assert red.bucket.is_cuda and all(torch.equal(red.params[i].grad, g) for i, g in before.items())
assert all(p.grad is not None for p in red.params)     # unused parameters received the reduced zeros
# one rank: SyncBatchNorm (statistics through RCCL) == stock BatchNorm
# (gradients of a bias in front of a BatchNorm are pure round-off in both: compare on the global gradient scale)
scale = max(q.grad.abs().max().item() for q in ref.parameters() if q.grad is not None)
worst = 0.0
for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
    if p.grad is not None and q.grad is not None:
        err = (p.grad - q.grad).abs().max().item() / scale
        worst = max(worst, err)
        assert err < 1e-4, (n, err)
t = torch.ones(4, device="cuda")
dist.all_reduce(t)
torch.cuda.synchronize()
assert t.sum().item() == 4.0

# a whole optimisation step -- SyncBatchNorm collectives, the gradient all-reduce (gradients are views of the flat
# bucket), Adam -- captured as ONE hipGraph and replayed; against the same step issued eagerly (same modules, same
# collectives).  The replayed steps must not synchronise with the host (sync debug mode "error" raises if they do).
from planar_optical_flow_amd.graph_step import GraphedTrainStep, make_capturable     # noqa: E402
torch.manual_seed(6)
gm = get_model(cfg).cuda()
pd.convert_sync_batchnorm(gm).train()
torch.manual_seed(6)
em = get_model(cfg).cuda()                      # the eager twin: the same modules, collectives issued eagerly
pd.convert_sync_batchnorm(em).train()
gopt = torch.optim.Adam(gm.parameters(), lr=1e-3, amsgrad=True)
eopt = torch.optim.Adam(em.parameters(), lr=1e-3, amsgrad=True)
ered = pd.GradientAllReduce(em, always=True)
make_capturable(gopt)
red2 = pd.GradientAllReduce(gm, always=True)
gstep = GraphedTrainStep(gm, gopt, {"input": x, "target": y}, reducer=red2)
assert gstep._fused_collective and len(gstep._graphs) == 1
assert all(p.grad.data_ptr() == v.data_ptr() for p, v in zip(red2.params, red2.views))
# The gradients are checked against a float64 CPU evaluation of the same step at the weights the step started from
# (stock BatchNorm == one-rank SyncBatchNorm), not against the eager twin: on these shapes MIOpen's timed solver choice
# sometimes picks a weight-gradient solver that computes conv4's weight gradient wrong in the EAGER step (2.25e-2 of
# scale on the fourth batch below; profiles/r3_graph_capture_miopen.txt), while the
# captured step is right on every solver.  The eager twin keeps MIOpen's default choice; its losses are compared, and
# its gradient deviation from the reference is reported.
cpu_ref = get_model(cfg).double().train()


def ref_grads(weights, xb, yb):
    with torch.no_grad():
        for p, w in zip(cpu_ref.parameters(), weights):
            p.copy_(w.double().cpu())
    cpu_ref.zero_grad(set_to_none=True)
    cpu_ref.loss_fn(cpu_ref(xb.double().cpu()), yb.double().cpu()).backward()
    return [p.grad for p in cpu_ref.parameters()]


def grad_err(m, ref):
    """worst |grad - reference| over the model, on the scale of the largest reference gradient (the gradients of a
    bias in front of a BatchNorm are pure round-off)"""
    rs = max(r.abs().max().item() for r in ref if r is not None)
    return max((p.grad.double().cpu() - r).abs().max().item() for p, r in zip(m.parameters(), ref)
               if r is not None and p.grad is not None) / rs


worst_loss = worst_graph = worst_eager = 0.0
for it in range(4):
    xb = torch.randn(12, 64, 3, device="cuda")
    yb = torch.randn(12, 3, device="cuda")
    red2.set_stop(it == 2)
    g_w = [p.detach().clone() for p in gm.parameters()]
    e_w = [p.detach().clone() for p in em.parameters()]
    torch.cuda.set_sync_debug_mode("error")
    gl = gstep({"input": xb, "target": yb})
    torch.cuda.set_sync_debug_mode("default")
    eopt.zero_grad(set_to_none=False)
    el = em.loss_fn(em(xb), yb)
    el.backward()
    ered()
    eopt.step()
    worst_loss = max(worst_loss, abs(gl.item() - el.item()) / max(abs(el.item()), 1e-6))
    assert red2.stop_requested() == (it == 2), it       # the flag of THIS step's all-reduce, read after it
    # this step's gradients (the graph's live in the flat bucket) against the reference at each model's own weights
    # (weights drift apart by round-off: where a gradient is pure round-off, Adam normalises it to steps of +-lr)
    gerr = grad_err(gm, ref_grads(g_w, xb, yb))
    assert gerr < 1e-4, (it, gerr)
    worst_graph = max(worst_graph, gerr)
    worst_eager = max(worst_eager, grad_err(em, ref_grads(e_w, xb, yb)))
assert worst_loss < 1e-5, worst_loss
dist.destroy_process_group()
print("RCCL_OK worst relative gradient difference SyncBN vs BatchNorm: %.2e; captured step with collectives: "
      "loss diff %.1e vs the eager twin, gradients %.1e of scale from the float64 reference (eager twin on MIOpen's "
      "default solvers: %.1e), no host sync in the replay" % (worst, worst_loss, worst_graph, worst_eager))
