"""Box-regression head training step with SyncBatchNorm on a one-rank `nccl` group (run on a GPU box): batch 256 x 64
points, forward + backward + gradient all-reduce + Adam, eager and as one hipGraph replay, timed with HIP events.

    python tools/bench_sync_bn_step.py                  # the HIP units with the global-batch tail (default route)
    python tools/bench_sync_bn_step.py --module-route   # the torch modules: library convolutions + dist._SyncBatchNormFn

Prints one JSON line."""
import argparse
import json
import os
import sys

import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "planar_optical_flow_amd"))
from planar_optical_flow_amd import dist as pd                                   # noqa: E402
from planar_optical_flow_amd.graph_step import GraphedTrainStep, make_capturable   # noqa: E402
from src.depracted.model.dr_spaam import DROW                                      # noqa: E402
from src.model.box_regression import PointNet                                      # noqa: E402
from src.model.get_model import get_model                                          # noqa: E402


def timed(fn, steps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--module-route", action="store_true")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29541")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    if a.module_route:
        PointNet.hip_sync_bn = DROW.hip_sync_bn = False
    cfg = {"type": "box_reg", "input_dim": 3, "target_dim": 3, "dropout": 0.3}
    g = torch.Generator(device="cuda").manual_seed(40)
    x = torch.randn((256, 64, 3), device="cuda", generator=g) * 0.3
    y = torch.randn((256, 3), device="cuda", generator=g) * 0.3

    torch.manual_seed(4)
    model = get_model(cfg).cuda()
    pd.convert_sync_batchnorm(model).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, amsgrad=True)
    red = pd.GradientAllReduce(model, always=True)

    def eager():
        opt.zero_grad(set_to_none=False)
        model.loss_fn(model(x), y).backward()
        red()
        opt.step()

    eager_ms = timed(eager, a.steps, a.warmup)

    torch.manual_seed(4)
    gm = get_model(cfg).cuda()
    pd.convert_sync_batchnorm(gm).train()
    gopt = torch.optim.Adam(gm.parameters(), lr=1e-3, amsgrad=True)
    make_capturable(gopt)
    gstep = GraphedTrainStep(gm, gopt, {"input": x, "target": y}, reducer=pd.GradientAllReduce(gm, always=True))
    batch = {"input": x, "target": y}
    graph_ms = timed(lambda: gstep(batch), a.steps, a.warmup)
    dist.destroy_process_group()
    print(json.dumps({"workload": "box head training step, SyncBatchNorm, one-rank nccl, batch 256 x 64 points",
                      "route": "torch modules" if a.module_route else "HIP units, global-batch tail",
                      "eager_ms_per_step": round(eager_ms, 4), "captured_ms_per_step": round(graph_ms, 4),
                      "steps": a.steps, "warmup": a.warmup}))


if __name__ == "__main__":
    main()
