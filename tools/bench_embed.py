"""The attention gate's embedding (K = 3584 -> E = 128): ``ops.attn_embed`` against the library route as the model issues
it -- F.linear + LeakyReLU on float32 rows, the slab-widening ``_embed_rows`` on float16 rows -- for one and two sources.
    python tools/bench_embed.py [R ...]          (default 450 3600 14400)
Same process, legs alternated, warm-up first, HIP events.  Prints time, TFLOP/s of the algorithm's 2 R K E per source and
the share of the float32-MFMA floor (157.3 TFLOP/s); for float16 rows also the peak allocation of one call."""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from planar_optical_flow_amd import ops  # noqa: E402
from planar_optical_flow_amd.src.depracted.model.dr_spaam import _SpatialAttention  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_embed.py measures on the GPU; there is no CPU figure")
dev = "cuda:0"
K, E, SLOPE, PEAK = 3584, 128, 0.1, 157.3e12
ROUNDS, CALLS = 5, 20


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / CALLS * 1e3                       # us per call


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - held


torch.manual_seed(7)
gate = _SpatialAttention(n_pts=14, n_channel=256).to(dev).eval()
with torch.no_grad():
    gate.conv[1].running_mean.normal_(0, 0.1)
    gate.conv[1].running_var.uniform_(0.5, 1.5)
gate.fold_for_inference(True)
w, b = gate._folded
print("form by rows:", {R: ops.attn_embed_plan(R, K, E) for R in (450, 3600, 8191, 8192, 14400)}, flush=True)
for R in ([int(v) for v in sys.argv[1:]] or [450, 3600, 14400]):
    for dtype in (torch.float32, torch.float16):
        x = torch.randn(R, K, device=dev).to(dtype)
        t = torch.randn(R, K, device=dev).to(dtype)
        for nsrc in (1, 2):
            srcs = (x, t)[:nsrc]
            with torch.no_grad():
                legs = {
                    "library": lambda: [gate._embed_rows(s) for s in srcs],
                    "hip": lambda: ops.attn_embed(x, t if nsrc == 2 else None, w, b, SLOPE),
                }
                lib, hip = legs["library"](), legs["hip"]()
                diff = max(float((a - c).abs().max()) for a, c in zip(lib, hip))
                for fn in legs.values():                             # warm-up: code objects, the library's solution
                    for _ in range(5):
                        fn()
                torch.cuda.synchronize()
                times = {name: [] for name in legs}
                for _ in range(ROUNDS):                              # alternate the legs
                    for name, fn in legs.items():
                        times[name].append(window(fn))
                mem = {name: peak_bytes(fn) for name, fn in legs.items()} if dtype == torch.float16 else None
            flop = 2.0 * R * K * E * nsrc
            for name in legs:
                ts = sorted(times[name])
                med = ts[len(ts) // 2]
                print("R=%5d %-7s sources=%d %-7s %8.1f us (min %.1f max %.1f)  %6.1f TFLOP/s  %5.1f %% of the float32-MFMA floor%s"
                      % (R, str(dtype).replace("torch.", ""), nsrc, name, med, ts[0], ts[-1], flop / med / 1e6,
                         100.0 * (flop / PEAK * 1e6) / med,
                         "" if mem is None else "  peak allocated %.1f MB" % (mem[name] / 1e6)), flush=True)
            print("R=%5d %-7s sources=%d max |hip - library| %.3e" % (R, str(dtype).replace("torch.", ""), nsrc, diff),
                  flush=True)
