"""DR-SPAAM forward (BASELINE config 3 shape): cutout -> SpatialDROW on the device.  Under rocprofv3
--kernel-trace --stats this shows how the time splits between the MIOpen trunks and the HIP kernels.
    python tools/bench_drspaam.py [B] [hip|torch|torch-find|train...] [--storage=float32|float16] [--embed=library|hip]
--storage=float16 (hip mode): float16 cutout and fuse_for_inference(storage=torch.float16); one storage type per
process.  --embed=hip (hip mode): the gate's embedding on ops.attn_embed instead of the library GEMM.  The hip mode also prints the forward in HIP-event time and the peak allocation of the timed forwards."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from planar_optical_flow_amd import ops, synth
from planar_optical_flow_amd.src.depracted.model.dr_spaam import SpatialDROW

STORAGE = [a.split("=", 1)[1] for a in sys.argv if a.startswith("--storage=")]
EMBED = ([a.split("=", 1)[1] for a in sys.argv if a.startswith("--embed=")] or ["library"])[0]
sys.argv = [a for a in sys.argv if not a.startswith(("--storage=", "--embed="))]
ACT = {"float32": torch.float32, "float16": torch.float16}[STORAGE[0] if STORAGE else "float32"]
B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
mode = sys.argv[2] if len(sys.argv) > 2 else "hip"      # hip | torch | torch-find
if mode == "torch-find":
    torch.backends.cudnn.benchmark = True               # MIOpen find mode instead of the immediate fallback
torch.manual_seed(3)
m = SpatialDROW(num_scans=5, num_pts=56, alpha=0.5, window_size=11, pedestrian_only=True).cuda().eval()
if mode == "hip":
    m.fuse_for_inference(storage=ACT, embed=EMBED)
elif ACT != torch.float32 or EMBED != "library":
    sys.exit("--storage=float16 and --embed=hip need the hip mode")
sb = synth.make_batch(seed=3, B=B, T=5)
scans = torch.from_numpy(sb.scans).cuda()
tab = ops.phi_table()
kw = dict(fixed=True, centered=True, window_width=1.0, window_depth=0.5, num_cutout_pts=56, padding_val=29.99,
          area_mode=True)
def step():
    x = ops.cutout(scans, tab, out_dtype=ACT, **kw)
    with torch.no_grad():
        return m(x)
if mode.startswith("train"):
    step = lambda: None
for _ in range(3): step()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(5): step()
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / 5
print("DR-SPAAM forward B=%d [%s]: %.2f ms/step  %.0f scans/s" % (B, mode, dt * 1e3, B / dt), flush=True)
if mode == "hip":
    out = None
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5): out = step()
    e1.record(); torch.cuda.synchronize()
    print("DR-SPAAM forward B=%d [hip, storage %s, embed %s]: %.3f ms/step (HIP events, 5 steps)  peak allocated %.1f MB "
          "(%.1f MB held before the step)  outputs finite: %s"
          % (B, ACT, EMBED, e0.elapsed_time(e1) / 5, torch.cuda.max_memory_allocated() / 1e6, held / 1e6,
             all(bool(torch.isfinite(o).all()) for o in out)), flush=True)
if mode in ("train", "train-miopen", "train-modules", "train-libconv"):
    # one optimisation-style step: forward in training mode (BatchNorm batch statistics) + backward
    m.train()
    m.fused_train_tail = mode != "train-modules"   # train-modules: the framework's own BatchNorm / LeakyReLU / pool
    m.hip_train_conv = mode != "train-libconv"       # train-libconv: MIOpen convolutions + the fused tail
    x = ops.cutout(scans, tab, **kw)
    def tstep():
        for p in m.parameters(): p.grad = None
        pc, pr, ff = m(x)
        (pc.sum() + pr.sum() + ff.sum()).backward()
    for _ in range(2): tstep()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5): tstep()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 5
    print("DR-SPAAM train step (fwd+bwd) B=%d [%s]: %.1f ms  peak mem %.1f GB" % (B, mode, dt * 1e3, torch.cuda.max_memory_allocated() / 1e9), flush=True)
