"""Streaming DR-SPAAM step latency (one scan per call): eager launches vs one hipGraph replay.
    python tools/bench_stream.py [B ...] [--embed=library|hip] [--storage=float32|float16] [--nms] [--flow=prototype|diff] [--ego[=scan_match|keyframe|keyframe_map]] [--tracks] [--person-motion] [--grid] [--grid-match] [--grid-refine] [--grid-scroll] [--grid-store] [--grid-cast] [--novel] [--merge] [--track-map]
--embed=hip: the gate's embedding on ops.attn_embed; --storage=float16 needs it (float16 cutout and template).
--nms: the centre NMS inside the step; --flow (implies --nms): the per-person flow as the step's tail, with a fused
Prototype or an elementwise scan difference as the flow model, a pose per scan.  --ego (with --flow): the replayed
step with a pose per scan against the step that dead-reckons its own pose (ego_motion=dict()), alternating repeats.
--tracks (with --flow): the replayed step without and with the person tracks (tracks=dict()) as its last node,
alternating repeats in one process; with --ego both dead-reckon their pose.
--ego=scan_match: the pose from the two scans alone (ego_motion=dict(method="scan_match")).  Without --flow: the bare
replayed step against the step that ends in the scan matcher and the pose; with --flow: pose per scan, the flow fit
and the scan matcher in front of the per-person flow, alternating repeats.
--ego=keyframe: as --ego=scan_match with the keyframe matcher (ego_motion=dict(method="keyframe")) as one more step
next to the scan matcher's, so one process gives the bare step, scan_match and keyframe.
--ego=keyframe_map: as --ego=keyframe with the keyframe map (ego_motion=dict(method="keyframe_map")) as one more step
next to the keyframe matcher's, so one process gives the bare step, scan_match, keyframe and keyframe_map.
--person-motion (with --ego=scan_match|keyframe|keyframe_map, without --flow; implies --nms for every step of the
process): two more steps next to those, the chosen method's with person_motion=dict() as its tail and that one with
tracks=dict() behind it, so one process gives the step without and with the person motion.
--grid (alone or with --nms): the replayed step with ego_motion=dict(method="keyframe") without and with
grid_map=dict() (512 x 512 cells of 0.1 m per sensor) as its last stage, alternating repeats in one process.
--grid-match (with --grid): two more steps in the same process, ego_motion=dict(method="scan_match") with grid_map=dict()
and that one with grid_match=dict() behind the scan matcher, so one process gives the map step without and with the
scan-to-grid match.
--grid-refine (with --grid): the scan_match + grid_map step (and with --grid-match the one with grid_match=dict()) once more
with grid_refine=dict() behind the pose launch, so one process gives those steps without and with the grid refine.
--grid-scroll (with --grid): one more step in the same process, the keyframe step with grid_map=dict() and
grid_scroll=dict() behind the keyframe launch, so one process gives the map step without and with the scrolling grid.
--grid-store (with --grid --grid-scroll): one more step in the same process, that step with grid_store=dict() -- the
scroll's entry of the stage table then calls the storing launch -- so one process gives the step without and with the
tile store behind the window.
--grid-cast (with --grid): one more step in the same process, the keyframe step with grid_map=dict() and
grid_cast=dict() directly in front of the grid map, so one process gives the map step without and with the ray cast.
--novel (with --grid; brings the --grid-cast step with it): one more step in the same process, that step with
novel_segments=dict() directly behind the cast, so one process gives the cast step without and with the novelty
segments.
--merge (with --grid --novel; implies --nms): instead of those steps, the keyframe step with grid_map=dict(),
grid_cast=dict(), novel_segments=dict(), person_motion=dict() and tracks=dict() without and with merge_detections=dict()
behind the segments, alternating repeats in one process.
--track-map (with --person-motion --tracks --grid, without --flow; --ego=scan_match|keyframe|keyframe_map chooses the
pose, keyframe by default): the replayed step with person_motion=dict(), tracks=dict() and grid_map=dict() without and
with track_map=dict() behind the grid map, alternating repeats in one process.
--eager (with --ego, --tracks or --grid): those steps launched eagerly (graph=False) instead of replayed -- the host
time of the stage wrappers, which a replay does not run."""
import faulthandler, os, sys, time
faulthandler.dump_traceback_later(90, exit=True)       # a stuck step reports where it is instead of hanging the box
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from planar_optical_flow_amd import synth
from planar_optical_flow_amd.streaming import StreamingDetector
from planar_optical_flow_amd.src.depracted.model.dr_spaam import SpatialDROW

EMBED = ([a.split("=", 1)[1] for a in sys.argv if a.startswith("--embed=")] or ["library"])[0]
STORAGE = ([a.split("=", 1)[1] for a in sys.argv if a.startswith("--storage=")] or ["float32"])[0]
FLOW = ([a.split("=", 1)[1] for a in sys.argv if a.startswith("--flow=")] or [None])[0]
PERSON_MOTION = "--person-motion" in sys.argv
NMS = 0.5 if (FLOW or "--nms" in sys.argv or PERSON_MOTION or "--merge" in sys.argv) else None
EGO_METHOD = ([a.split("=", 1)[1] for a in sys.argv if a.startswith("--ego=")] or ["flow"])[0]
EGO = any(a == "--ego" or a.startswith("--ego=") for a in sys.argv)
MATCH = dict(method="scan_match")
KEYFRAME = dict(method="keyframe")
KEYFRAME_MAP = dict(method="keyframe_map")
KEYED = ("keyframe", "keyframe_map")
TRACKS = "--tracks" in sys.argv
GRID = "--grid" in sys.argv
GRID_MATCH = "--grid-match" in sys.argv
GRID_REFINE = "--grid-refine" in sys.argv
GRID_SCROLL = "--grid-scroll" in sys.argv
GRID_STORE = "--grid-store" in sys.argv
GRID_CAST = "--grid-cast" in sys.argv
NOVEL = "--novel" in sys.argv
MERGE = "--merge" in sys.argv
if MERGE and not (GRID and NOVEL):
    sys.exit("--merge needs --grid --novel")
TRACK_MAP = "--track-map" in sys.argv
if TRACK_MAP and not (PERSON_MOTION and TRACKS and GRID and FLOW is None):
    sys.exit("--track-map needs --person-motion --tracks --grid and no --flow")
EAGER = "--eager" in sys.argv
sys.argv = [a for a in sys.argv if not a.startswith(("--embed=", "--storage=", "--flow=", "--nms", "--ego", "--tracks", "--track-map", "--person-motion", "--grid", "--novel", "--merge", "--eager"))]


class DiffFlow(torch.nn.Module):
    def forward(self, prev, cur):
        d = (cur - prev)[..., 0]
        return torch.stack((d, 0.5 * d), dim=-1)


flow_model = None
if FLOW == "prototype":
    from planar_optical_flow_amd.src.depracted.model.prototype import Prototype
    flow_model = Prototype(in_channel=1, max_displacement=5).cuda().eval().fuse_for_inference()
elif FLOW == "diff":
    flow_model = DiffFlow()
torch.manual_seed(3)
model = SpatialDROW(num_scans=5, num_pts=56, alpha=0.5, window_size=11, pedestrian_only=True).cuda().eval()
model.fuse_for_inference(storage={"float32": torch.float32, "float16": torch.float16}[STORAGE], embed=EMBED)
for B in ([int(v) for v in sys.argv[1:]] or [1, 8]):
    scans = torch.from_numpy(synth.make_batch(seed=9, B=B, T=40).scans).cuda()     # [B, 40, 450]
    if EGO or TRACKS or GRID:
        poses = np.cumsum(np.random.default_rng(4).normal(0, 0.05, (40, B, 3)), axis=0)
        mk = lambda **kw: StreamingDetector(model, batch=B, nms_min_dist=NMS, flow_model=flow_model, graph=not EAGER, **kw)
        if TRACK_MAP:
            chain = dict(ego_motion={"scan_match": MATCH, "keyframe_map": KEYFRAME_MAP}.get(EGO_METHOD, KEYFRAME),
                         person_motion=dict(), tracks=dict(), grid_map=dict())
            unchecked, checked = mk(**chain), mk(track_map=dict(), **chain)
            steps = {"person_motion + tracks + grid_map": lambda t: unchecked(scans[:, t]),
                     "person_motion + tracks + grid_map + track_map": lambda t: checked(scans[:, t])}
        elif MERGE:
            chain = dict(ego_motion=KEYFRAME, grid_map=dict(), grid_cast=dict(), novel_segments=dict(),
                         person_motion=dict(), tracks=dict())
            apart, merged = mk(**chain), mk(merge_detections=dict(), **chain)
            steps = {"grid_map + grid_cast + novel_segments + person_motion + tracks": lambda t: apart(scans[:, t]),
                     "the same + merge_detections": lambda t: merged(scans[:, t])}
        elif GRID:
            keyed_only, gridded = mk(ego_motion=KEYFRAME), mk(ego_motion=KEYFRAME, grid_map=dict())
            steps = {"keyframe": lambda t: keyed_only(scans[:, t]), "keyframe + grid_map": lambda t: gridded(scans[:, t])}
            if GRID_SCROLL:
                scrolling = mk(ego_motion=KEYFRAME, grid_map=dict(), grid_scroll=dict())
                steps["keyframe + grid_map + grid_scroll"] = lambda t: scrolling(scans[:, t])
            if GRID_SCROLL and GRID_STORE:
                storing = mk(ego_motion=KEYFRAME, grid_map=dict(), grid_scroll=dict(), grid_store=dict())
                steps["keyframe + grid_map + grid_scroll + grid_store"] = lambda t: storing(scans[:, t])
            if GRID_CAST or NOVEL:
                casting = mk(ego_motion=KEYFRAME, grid_map=dict(), grid_cast=dict())
                steps["keyframe + grid_map + grid_cast"] = lambda t: casting(scans[:, t])
            if NOVEL:
                grouping = mk(ego_motion=KEYFRAME, grid_map=dict(), grid_cast=dict(), novel_segments=dict())
                steps["keyframe + grid_map + grid_cast + novel_segments"] = lambda t: grouping(scans[:, t])
            if GRID_MATCH:
                reckoned, corrected = mk(ego_motion=MATCH, grid_map=dict()), mk(ego_motion=MATCH, grid_map=dict(), grid_match=dict())
                steps["scan_match + grid_map"] = lambda t: reckoned(scans[:, t])
                steps["scan_match + grid_map + grid_match"] = lambda t: corrected(scans[:, t])
            if GRID_REFINE:
                if not GRID_MATCH:
                    reckoned = mk(ego_motion=MATCH, grid_map=dict())
                    steps["scan_match + grid_map"] = lambda t: reckoned(scans[:, t])
                kw = dict(grid_match=dict()) if GRID_MATCH else {}
                refined = mk(ego_motion=MATCH, grid_map=dict(), grid_refine=dict(), **kw)
                steps["scan_match + grid_map + %sgrid_refine" % ("grid_match + " if GRID_MATCH else "")] = lambda t: refined(scans[:, t])
        elif TRACKS:
            kw = dict(ego_motion={"scan_match": MATCH, "keyframe": KEYFRAME, "keyframe_map": KEYFRAME_MAP}.get(EGO_METHOD, dict())) if EGO else {}
            plain, tracked = mk(tracks=None, **kw), mk(tracks=dict(), **kw)
            call = (lambda det, t: det(scans[:, t])) if EGO else (lambda det, t: det(scans[:, t], pose=poses[t]))
            steps = {"tracks=None": lambda t: call(plain, t), "tracks": lambda t: call(tracked, t)}
        elif EGO_METHOD in ("scan_match",) + KEYED and flow_model is None:
            bare, matched = mk(), mk(ego_motion=MATCH)
            steps = {"no pose": lambda t: bare(scans[:, t]), "scan_match": lambda t: matched(scans[:, t])}
            if EGO_METHOD in KEYED:
                keyed = mk(ego_motion=KEYFRAME)
                steps["keyframe"] = lambda t: keyed(scans[:, t])
            if EGO_METHOD == "keyframe_map":
                mapped = mk(ego_motion=KEYFRAME_MAP)
                steps["keyframe_map"] = lambda t: mapped(scans[:, t])
            if PERSON_MOTION:
                chosen = {"scan_match": MATCH, "keyframe": KEYFRAME, "keyframe_map": KEYFRAME_MAP}[EGO_METHOD]
                moved = mk(ego_motion=chosen, person_motion=dict())
                followed = mk(ego_motion=chosen, person_motion=dict(), tracks=dict())
                steps[EGO_METHOD + " + person_motion"] = lambda t: moved(scans[:, t])
                steps[EGO_METHOD + " + person_motion + tracks"] = lambda t: followed(scans[:, t])
        else:
            posed, ego = mk(), mk(ego_motion=dict())
            steps = {"pose=": lambda t: posed(scans[:, t], pose=poses[t]), "ego_motion": lambda t: ego(scans[:, t])}
            if EGO_METHOD in ("scan_match",) + KEYED:
                matched = mk(ego_motion=MATCH)
                steps["scan_match"] = lambda t: matched(scans[:, t])
            if EGO_METHOD in KEYED:
                keyed = mk(ego_motion=KEYFRAME)
                steps["keyframe"] = lambda t: keyed(scans[:, t])
            if EGO_METHOD == "keyframe_map":
                mapped = mk(ego_motion=KEYFRAME_MAP)
                steps["keyframe_map"] = lambda t: mapped(scans[:, t])
        for step in steps.values():
            for t in range(8):
                step(t)
        ms = {k: [] for k in steps}
        for rep in range(4):
            for name, step in steps.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for t in range(8, 40):
                    step(t)
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) / 32 * 1e3)
        if TRACK_MAP:
            live, _, state, out = checked.track_map()
            print("   track_map after 40 scans: live tracks %s, with evidence %s, classes (0-3) %s"
                  % ([len(l) for l in live], (state.ev_scans > 0).sum(dim=1).tolist(), out.class_count.tolist()))
            print("streaming step B=%d, %s per scan, 4 alternating repeats of 32 steps: %s"
                  % (B, "eager launches" if EAGER else "hipGraph replay",
                     ", ".join("%s %s ms" % (k, " ".join("%.3f" % v for v in vs)) for k, vs in ms.items())), flush=True)
            continue
        if MERGE:
            o = merged.merged_detections()
            print("   merge_detections at the last scan: (NMS rows, appended, absorbed, dropped) %s; live tracks %s without, "
                  "%s with" % (o.merge_count.tolist(), [len(l) for l in apart.tracks()[0]],
                               [len(l) for l in merged.tracks()[0]]))
            print("streaming step B=%d, %s per scan, 4 alternating repeats of 32 steps: %s"
                  % (B, "eager launches" if EAGER else "hipGraph replay",
                     ", ".join("%s %s ms" % (k, " ".join("%.3f" % v for v in vs)) for k, vs in ms.items())), flush=True)
            continue
        if EGO_METHOD == "keyframe_map" and not TRACKS:
            fits, _ = mapped.ego_motion()
            print("   keyframe_map at the last scan: iterations %s, matched %s, ok %s, key age %s, slot %s"
                  % ([f["iters_used"] for f in fits], [f["count"] for f in fits], [f["ok"] for f in fits],
                     [f["key_age"] for f in fits], [f["key_slot"] for f in fits]))
        if EGO_METHOD in KEYED and not TRACKS:
            fits, _ = keyed.ego_motion()
            print("   keyframe at the last scan: iterations %s, matched %s, ok %s, key age %s"
                  % ([f["iters_used"] for f in fits], [f["count"] for f in fits], [f["ok"] for f in fits],
                     [f["key_age"] for f in fits]))
        if EGO_METHOD in ("scan_match",) + KEYED and not TRACKS:
            fits, _ = matched.ego_motion()
            print("   scan_match at the last scan: iterations %s, matched %s, ok %s"
                  % ([f["iters_used"] for f in fits], [f["count"] for f in fits], [f["ok"] for f in fits]))
        if PERSON_MOTION and EGO_METHOD in ("scan_match",) + KEYED and flow_model is None:
            people, _ = moved.person_motion()
            live, _, state = followed.tracks()
            print("   person_motion at the last scan: detections %s, paired %s; tracks: %s live, next_id %s"
                  % ([len(p["prev"]) for p in people], [int((p["prev"] >= 0).sum()) for p in people],
                     [len(l) for l in live], state.next_id.tolist()))
        if GRID:
            state, out = gridded.grid_map()
            print("   grid_map after 40 scans: occupied cells %s, free cells %s, marked points of the last scan %s"
                  % ((state.grid > 0).sum(dim=(1, 2)).tolist(), (state.grid < 0).sum(dim=(1, 2)).tolist(),
                     out.point_mark.sum(dim=1).tolist()))
        if GRID and GRID_SCROLL:
            moved_by, _ = scrolling.grid_scroll()
            print("   grid_scroll at the last scan: shift %s, offset %s" % ([m["shift"].tolist() for m in moved_by],
                                                                             [m["offset"].tolist() for m in moved_by]))
        if GRID and GRID_SCROLL and GRID_STORE:
            print("   grid_store at the last scan: %s" % storing.grid_store()[0])
        if GRID and (GRID_CAST or NOVEL):
            o = casting.grid_cast()
            print("   grid_cast at the last scan: points per class (none, map, novel, through, unknown) %s, cells read %s"
                  % (o.class_count.tolist(), o.exp_steps.sum(dim=1).tolist()))
        if GRID and NOVEL:
            o = grouping.novel_segments()
            print("   novel_segments at the last scan: segments (all, few, wide) %s, kept %s, NOVEL points %s"
                  % (o.seg_count.tolist(), o.num_det.tolist(), grouping.grid_cast().class_count[:, 2].tolist()))
        if GRID and GRID_MATCH:
            found, _ = corrected.grid_match()
            print("   grid_match at the last scan: votes %s, score per voting point %s, ok %s, moved %s"
                  % ([f["votes"] for f in found], ["%.1f" % (f["score"][0] / max(f["votes"], 1)) for f in found],
                     [f["ok"] for f in found], [f["moved"] for f in found]))
        if GRID and GRID_REFINE:
            found, _ = refined.grid_refine()
            print("   grid_refine at the last scan: votes %s, inside %s, updates %s, score before and after %s, ok %s, moved %s"
                  % ([f["votes"] for f in found], [f["count"] for f in found], [f["iters_used"] for f in found],
                     [["%.3f" % v for v in f["score"]] for f in found], [f["ok"] for f in found], [f["moved"] for f in found]))
        if TRACKS and not GRID:
            live, _, state = tracked.tracks()
            print("   tracks after 40 scans: %s live, next_id %s" % ([len(l) for l in live], state.next_id.tolist()))
        print("streaming step B=%d [flow %s%s], %s per scan, 4 alternating repeats of 32 steps: %s"
              % (B, FLOW, ", ego" if EGO and TRACKS else "", "eager launches" if EAGER else "hipGraph replay", ", ".join("%s %s ms" % (k, " ".join("%.3f" % v for v in vs)) for k, vs in ms.items())), flush=True)
        continue
    res = {}
    for graph in (False, True):
        det = StreamingDetector(model, batch=B, graph=graph, nms_min_dist=NMS, flow_model=flow_model)
        poses = np.cumsum(np.random.default_rng(4).normal(0, 0.05, (40, B, 3)), axis=0)
        step = (lambda t: det(scans[:, t], pose=poses[t])) if flow_model is not None else (lambda t: det(scans[:, t]))
        outs = []
        for t in range(8):
            cls, reg = step(t)
            outs.append((cls.clone(), reg.clone()))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(8, 40):
            step(t)
        torch.cuda.synchronize()
        res[graph] = ((time.perf_counter() - t0) / 32 * 1e3, outs)
    same = all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(res[False][1], res[True][1]))
    print("streaming step B=%d [embed %s, storage %s, nms %s, flow %s]: eager %.3f ms, hipGraph replay %.3f ms per scan (identical outputs: %s)"
          % (B, EMBED, STORAGE, NMS, FLOW, res[False][0], res[True][0], same), flush=True)
