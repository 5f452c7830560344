"""Map-checked tracks (pof_track_map, N15) on the GPU: the device against the NumPy restatement of
tests/test_track_map.py, every state field and every output BIT FOR BIT after every step (integers throughout; the one
float64 expression, the travel test, is plain multiplies and adds) -- on the rule scenes, on ray-cast rooms with people
fed by the device's own track_update and grid_map_update, on random legal inputs at both launch forms and both slot
counts per lane; at five batch positions, in two runs and in two replays of a captured step; refused calls; through
``utils.TrackMap``; and as a stage of the streaming detector, eager and replayed."""
import os
import sys

import numpy as np
import pytest
import torch

from test_person_motion import people_scene
from test_scan_match import trajectory
from test_track_map import (DEFAULTS, INPUTS, OUT_DTYPES, OUT_FIELDS, STATE_DTYPES, STATE_FIELDS, new_state,
                            random_scene, rule_scenes, run_steps, same_bits, track_map_oracle)

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "planar_optical_flow_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

FIELDS = STATE_FIELDS + OUT_FIELDS
DTYPES = STATE_DTYPES + OUT_DTYPES


@pytest.fixture(scope="module")
def ops():
    from planar_optical_flow_amd import ops as _ops
    return _ops


def _records(ops, steps):
    """One step of B sensors (the dicts of tests/test_track_map) as the records the wrapper takes: a TrackState and a
    GridMapOut whose other fields are zeros, and the NMS results."""
    stack = lambda k, dt: torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(s[k]) for s in steps]), dtype=dt)).cuda()
    B, M, N = len(steps), len(steps[0]["track_id"]), len(steps[0]["inst"])
    tracks = ops.track_buffers(B, M, N)._replace(track_id=stack("track_id", np.int32),
                                                 track_state=stack("track_state", np.float64),
                                                 track_det=stack("track_det", np.int32))
    seen = ops.grid_map_buffers(B, N)._replace(point_cell=stack("point_cell", np.int32),
                                               point_prior=stack("point_prior", np.int16),
                                               det_points=stack("det_points", np.int32),
                                               det_free=stack("det_free", np.int32))
    return tracks, seen, stack("inst", np.int32), stack("num_det", np.int32)


def _state(ops, sensors):
    M = len(sensors[0]["steps"][0]["track_id"])
    state = ops.track_map_state(len(sensors), M)
    for b, scene in enumerate(sensors):
        for k, v in scene.get("init", {}).items():
            getattr(state, k)[b].copy_(torch.from_numpy(np.asarray(v, new_state(M)[k].dtype)))
    return state


def _host(state, out):
    return {k: t.cpu().numpy() for k, t in list(zip(STATE_FIELDS, state)) + list(zip(OUT_FIELDS, out))}


def dev_steps(ops, sensors):
    """The device's state and outputs after every step, the sensors (scenes with the same sizes and settings) in one
    batch."""
    first = sensors[0]["steps"][0]
    state = _state(ops, sensors)
    out, res = ops.track_map_buffers(len(sensors), len(first["track_id"]), len(first["inst"])), []
    for steps in zip(*[s["steps"] for s in sensors]):
        ops.track_map(*_records(ops, steps), state, out=out, **sensors[0]["kw"])
        res.append(_host(state, out))
    return res


def check(ops, sensors, what):
    got = dev_steps(ops, sensors)
    decided = 0
    for b, scene in enumerate(sensors):
        for t, want in enumerate(run_steps(scene)):
            for k, dt in zip(FIELDS, DTYPES):
                assert got[t][k].dtype == dt and same_bits(got[t][k][b], want[k]), (what, b, t, k)
            decided += int((want["track_class"] != 0).sum())
    print("%s: %d sensors x %d steps, %d decided classes in all, every field the restatement's bits"
          % (what, len(sensors), len(sensors[0]["steps"]), decided))
    return got


# ------------------------------------------------------------------ 1. the device against the restatement
@pytest.mark.parametrize("name", sorted(rule_scenes()))
def test_rule_scenes(ops, name):
    check(ops, [rule_scenes()[name]], name)


SHAPES = {"64 x 4": (64, 4, True), "512 x 64": (512, 64, False), "513 x 65": (513, 65, False),
          "4096 x 256": (4096, 256, False)}


def random_sensors(name, seeds=(1, 2, 3), T=16):
    N, M, every_row = SHAPES[name]
    return [random_scene(1000 * N + seed, N, M, T, every_row=every_row, **(dict(min_points=3) if every_row else {}))
            for seed in seeds]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_random_legal_inputs(ops, name):
    got = check(ops, random_sensors(name), name)
    classes = np.concatenate([g["track_class"].reshape(-1) for g in got])
    assert (classes == 1).any() and (classes == 3).any() and got[-1]["ev_moved"].any()


CHAIN_SEEDS, CHAIN_T, CHAIN_M, CHAIN_SIDE, CHAIN_RES = (1, 2, 3), 6, 16, 256, 0.1


def test_rooms_with_people_fed_by_the_device_stages(ops):
    """N = 450, B = 3, 6 scans: person_motion, track_update and grid_map_update run on the device, and after every scan
    the restatement is applied to what they left there."""
    scenes = [people_scene(seed, CHAIN_T, 0.06) for seed in CHAIN_SEEDS]
    B, N = len(scenes), 450
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
    stack = lambda t, k, dt: dev(np.stack([sc["scans"][t][k] for sc in scenes]), dt)
    tab = dev(scenes[0]["tab"], np.float64)
    pm, tracks = ops.person_motion_state(B, N), ops.track_buffers(B, CHAIN_M, N)
    grid = ops.grid_map_reset(ops.grid_map_state(B, CHAIN_SIDE, CHAIN_SIDE),
                              dev(np.stack([sc["poses"][0, :2] for sc in scenes]) - 0.5 * CHAIN_RES * CHAIN_SIDE, np.float64))
    state, want = ops.track_map_state(B, CHAIN_M), [new_state(CHAIN_M) for _ in range(B)]
    added = 0
    for t in range(CHAIN_T):
        ranges, inst, num = stack(t, "ranges", np.float32), stack(t, "inst", np.int32), stack(t, "num_det", np.int32)
        det_xy, det_cls = stack(t, "det_xy", np.float64), stack(t, "det_cls", np.float64)
        rot, trans = stack(t, "rot", np.float32), stack(t, "trans", np.float64)
        o = ops.person_motion(ranges, tab, inst, num, det_xy, det_cls, rot, trans, pm)
        ops.track_update(o.det_xy_world, o.det_flow, o.det_valid, num, inst, tracks)
        seen = ops.grid_map_update(ranges, tab, rot, trans, grid, res=CHAIN_RES, instance_mask=inst, num_det=num,
                                   det_cls=det_cls)
        out = ops.track_map(tracks, seen, inst, num, state)
        got = _host(state, out)
        h = {k: getattr(seen, k).cpu().numpy() for k in ("point_cell", "point_prior", "det_points", "det_free")}
        h.update({k: getattr(tracks, k).cpu().numpy() for k in ("track_id", "track_state", "track_det")})
        for b in range(B):
            w = track_map_oracle(inst[b].cpu().numpy(), int(num[b]), *[h[k][b] for k in INPUTS[2:]], want[b], **DEFAULTS)
            for k in FIELDS:
                assert same_bits(got[k][b], dict(w, **want[b])[k]), (t, b, k)
        added += int((got["ev_scans"] > 0).sum())
    assert (got["ev_scans"] == CHAIN_T).any() and (got["track_class"] != 0).any() and got["ev_free"].any()
    print("rooms: %d live slots with evidence at the last scan, classes %s"
          % (int((got["ev_scans"] > 0).sum()), np.bincount(got["track_class"].reshape(-1), minlength=4).tolist()))


# ------------------------------------------------------------------ 2. determinism
def test_same_bits_at_five_batch_positions_and_in_two_runs(ops):
    me, other = random_sensors("513 x 65", seeds=(7, 8), T=8)
    want = run_steps(me)
    runs = []
    for pos in list(range(5)) + [2]:
        sensors = [other] * 5
        sensors[pos] = me
        got = dev_steps(ops, sensors)
        for t, w in enumerate(want):
            for k in FIELDS:
                assert same_bits(got[t][k][pos], w[k]), (pos, t, k)
        runs.append(got)
    for k in FIELDS:                                           # the two runs at position 2: every sensor's bits
        assert all(same_bits(a[k], b[k]) for a, b in zip(runs[2], runs[5])), k


def test_two_replays_of_a_captured_step_with_a_reset_in_between(ops):
    sensors = random_sensors("512 x 64", T=8)
    want = dev_steps(ops, sensors)                             # the eager run
    steps = [_records(ops, s) for s in zip(*[sc["steps"] for sc in sensors])]
    tracks, seen, inst, num = [r._replace(**{k: torch.zeros_like(v) for k, v in r._asdict().items()})
                               if hasattr(r, "_replace") else torch.zeros_like(r) for r in steps[0]]
    state, out = _state(ops, sensors), ops.track_map_buffers(len(sensors), 64, 512)
    kw = sensors[0]["kw"]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                              # warm-up on a state of its own
        ops.track_map(tracks, seen, inst, num, _state(ops, sensors), **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.track_map(tracks, seen, inst, num, state, out=out, **kw)
    for _ in range(2):
        ops.track_map_reset(state)
        assert not any(t.any() for t in state)
        for t, (tr, se, i, n) in enumerate(steps):
            for dst, src in list(zip(tracks, tr)) + list(zip(seen, se)) + [(inst, i), (num, n)]:
                dst.copy_(src)
            graph.replay()
            got = _host(state, out)
            for k in FIELDS:
                assert same_bits(got[k], want[t][k]), (t, k)


# ------------------------------------------------------------------ 3. refused calls
def test_refused_calls_leave_state_and_outputs_untouched(ops):
    from planar_optical_flow_amd._lib import POF_E_SHAPE, PofError
    rng = np.random.default_rng(1)
    cases = ((4097, 4, dict(cap=4097), PofError), (64, 257, {}, PofError), (64, 4, dict(cap=63), AssertionError),
             (64, 4, dict(free_pct=101), AssertionError), (64, 4, dict(travel=-1.0), AssertionError),
             (64, 4, dict(occ_pct=-1), AssertionError), (64, 4, dict(occ_thresh=-1), AssertionError),
             (64, 4, dict(min_scans=-1), AssertionError), (64, 4, dict(cap=(1 << 20) + 1), AssertionError),
             (64, 4, dict(travel=float("nan")), AssertionError), (4097, 4, {}, AssertionError))    # cap < N comes first
    for N, M, kw, error in cases:
        step = random_scene(5, N, M, 1)["steps"][0]
        state, out = ops.track_map_state(1, M), ops.track_map_buffers(1, M, N)
        for t in tuple(state) + tuple(out):                    # sentinels
            t.copy_(torch.from_numpy(rng.integers(1, 100, tuple(t.shape))).to(t.dtype))
        before = [t.cpu().numpy() for t in tuple(state) + tuple(out)]
        with pytest.raises(error) as e:
            ops.track_map(*_records(ops, [step]), state, out=out, **dict(DEFAULTS, **kw))
        if error is PofError:
            assert e.value.code == POF_E_SHAPE
        torch.cuda.synchronize()
        after = [t.cpu().numpy() for t in tuple(state) + tuple(out)]
        assert all(np.array_equal(a, b) for a, b in zip(before, after)), (N, M, kw)
    scene = random_scene(5, 64, 4, 2)
    records = _records(ops, [scene["steps"][0]])
    with pytest.raises(ValueError):
        ops.track_map(*records, ops.track_map_state(2, 4))     # the state of another batch
    with pytest.raises(ValueError):
        ops.track_map(*records, ops.track_map_state(1, 5))     # of another slot count
    with pytest.raises(ValueError):
        ops.track_map(*records, ops.track_map_state(1, 4), out=ops.track_map_buffers(1, 4, 65))
    with pytest.raises(ValueError):
        ops.track_map(records[0], records[1], records[2][:, :63].contiguous(), records[3], ops.track_map_state(1, 4))
    empty = ops.track_map(ops.track_buffers(0, 4, 64), ops.grid_map_buffers(0, 64), records[2][:0], records[3][:0],
                          ops.track_map_state(0, 4))
    assert empty.det_class.shape == (0, 64) and empty.class_count.shape == (0, 4)
    check(ops, [scene], "the next good call")


# ------------------------------------------------------------------ 4. the reference-shaped wrapper
def test_track_map_wrapper_equals_the_direct_calls(ops):
    import src.utils.utils as u
    scene = people_scene(24, 5, 0.2)
    N, res, size, M = 450, 0.1, 128, 32
    phi = scene["tab"][:N]
    rng = np.random.default_rng(3)
    settings = dict(min_points=5, min_scans=2)
    pm, tracker = u.PersonMotion(phi, max_range=10.0), u.PersonTracker(max_tracks=M)
    og, tm = u.OccupancyGrid(phi, res=res, size=size, max_range=10.0), u.TrackMap(max_tracks=M, **settings)
    tab = u._table_for(phi)
    motion, tracks, ev = ops.person_motion_state(1, N), ops.track_buffers(1, M, N), ops.track_map_state(1, M)
    grid = ops.grid_map_reset(ops.grid_map_state(1, size, size), scene["poses"][0][:2] - 0.5 * res * size)
    cls, reg = rng.uniform(0.05, 0.95, (N, 1)), rng.normal(0.0, 0.05, (N, 2))
    with pytest.raises(ValueError):
        tm.update(tracker, og)                                 # nothing to join yet
    decided = 0
    for t, s in enumerate(scene["scans"]):
        result = pm.update(s["ranges"], cls, reg, scene["poses"][t])
        tracker.update(result)
        og.update(s["ranges"], scene["poses"][t], cls, reg)
        got = tm.update(tracker, og)
        ranges = torch.from_numpy(s["ranges"]).cuda().reshape(1, N)
        xy, dc, num, inst = ops.nms_predicted_center(ranges, tab, torch.from_numpy(cls[:, 0].copy()).cuda().reshape(1, N),
                                                     torch.from_numpy(reg).cuda().reshape(1, N, 2), 0.5)
        rot, trans, _ = u._pose_terms(scene["poses"][t][None])
        rot, trans = torch.from_numpy(rot).cuda(), torch.from_numpy(trans).cuda()
        o = ops.person_motion(ranges, tab, inst, num, xy, dc, rot, trans, motion, max_range=10.0)
        ops.track_update(o.det_xy_world, o.det_flow, o.det_valid, num, inst, tracks)
        seen = ops.grid_map_update(ranges, tab, rot, trans, grid, res=res, max_range=10.0, instance_mask=inst,
                                   num_det=num, det_cls=dc)
        out = ops.track_map(tracks, seen, inst, num, ev, **settings)
        live, m = np.flatnonzero(tracks.track_id[0].cpu().numpy()), int(num[0])
        for key, t_ in (("id", tracks.track_id), ("cls", out.track_class), ("points", ev.ev_points), ("free", ev.ev_free),
                        ("occ", ev.ev_occ), ("scans", ev.ev_scans), ("start", ev.ev_start)):
            assert same_bits(got[key], t_[0].cpu().numpy()[live]), (t, key)
        assert np.array_equal(got["moved"], ev.ev_moved[0].cpu().numpy()[live].astype(bool)) and got["moved"].dtype == bool
        assert np.array_equal(got["det_class"], out.det_class[0, :m].cpu().numpy()) and len(got["det_class"]) == m
        assert np.array_equal(got["point_class"], out.point_class[0].cpu().numpy())
        assert np.array_equal(got["class_count"], out.class_count[0].cpu().numpy())
        decided += int((got["cls"] != 0).sum())
    assert len(got["id"]) > 0 and decided > 0
    tm.reset()
    assert not tm.update(tracker, og)["scans"].max() > 1       # evidence starts again
    with pytest.raises(ValueError):
        u.TrackMap(max_tracks=M + 1).update(tracker, og)       # another slot count than the tracker's
    with pytest.raises(ValueError):
        u.TrackMap(min_point=3)


# ------------------------------------------------------------------ 5. streaming detector
def _stream_model(seed):
    from planar_optical_flow_amd.src.depracted.model.dr_spaam import SpatialDROW
    torch.manual_seed(seed)
    return SpatialDROW(num_scans=5, num_pts=56, alpha=0.5, window_size=11, pedestrian_only=True).cuda().eval()


def _snapshot(det, stage):
    """What the stage reads and leaves behind (``stage``), and every other accessor's records, on the host."""
    _, conf, num, inst = det._dets
    snap = {"pred_cls": det.pred_cls, "pred_reg": det.pred_reg, "det_cls": conf, "num_det": num, "inst": inst,
            "rot": det._pose_rot, "trans": det._pose_trans, "grid": det._gm_state.grid, "origin": det._gm_state.origin}
    snap.update(det._gm_out._asdict())
    snap.update(det._track_state._asdict())
    snap.update({"pm_" + k: v for k, v in det._pm_out._asdict().items()})
    if det._dead_reckons():
        snap["pose"] = det._pose_state
    if stage:
        snap.update(det._tm_state._asdict())
        snap.update(det._tm_out._asdict())
    return {k: v.detach().cpu().numpy().copy() for k, v in snap.items()}


@pytest.mark.parametrize("ego", ["keyframe", "scan_match"])
def test_streaming_detector_eager_graph_and_restatement(ego):
    from planar_optical_flow_amd.streaming import StreamingDetector
    B, T, M = 2, 6, 64
    scans, _ = trajectory(T, B, seed=71, noise=0.01)
    model = _stream_model(13)
    kw = dict(batch=B, nms_min_dist=0.5, cls_thresh=0.5, ego_motion=dict(method=ego), person_motion=dict(),
              tracks=dict(), grid_map=dict(size=128))
    eager = StreamingDetector(model, graph=False, track_map=dict(), **kw)
    graphed = StreamingDetector(model, graph=True, track_map=dict(), **kw)
    parent = StreamingDetector(model, graph=True, **kw)        # what the detector was without the stage
    assert parent._tm_kw is None and not hasattr(parent, "_tm_state") and not hasattr(parent, "_tm_out")
    assert len(eager._stages) == len(parent._stages) + 1 and eager._tm_kw == DEFAULTS
    assert eager._stages[-2].launch == eager._track_map_stage and eager._stages[-1].launch == eager._keep_scan \
        if ego == "scan_match" else eager._stages[-1].launch == eager._track_map_stage

    def run():
        want = [new_state(M) for _ in range(B)]
        for det in (eager, graphed, parent):
            det.reset(pose=(0.213, -0.127, 0.3))
        for t in range(T):
            for det in (eager, graphed, parent):
                det(torch.from_numpy(scans[t]).cuda())
                if t == 0 and det is not parent:
                    with pytest.raises(RuntimeError):
                        det.track_map()
            e, g, p = _snapshot(eager, True), _snapshot(graphed, True), _snapshot(parent, False)
            for k in e:
                assert same_bits(e[k], g[k]), (t, k)           # eager and replayed: identical bits
            for k in p:
                assert same_bits(p[k], g[k]), (t, k)           # every other record: the detector's without the stage
            for b in range(B):
                w = track_map_oracle(g["inst"][b], g["num_det"][b], *[g[k][b] for k in INPUTS[2:]], want[b], **DEFAULTS)
                for k in FIELDS:
                    assert same_bits(g[k][b], dict(w, **want[b])[k]), (t, b, k)
        live, det_class, state, out = graphed.track_map()
        assert state is graphed._tm_state and out is graphed._tm_out and len(live) == B == len(det_class)
        for b in range(B):
            slots = np.flatnonzero(g["track_id"][b])
            assert [d["id"] for d in live[b]] == g["track_id"][b][slots].tolist()
            assert [d["cls"] for d in live[b]] == g["track_class"][b][slots].tolist()
            assert [d["points"] for d in live[b]] == g["ev_points"][b][slots].tolist()
            assert [d["moved"] for d in live[b]] == g["ev_moved"][b][slots].astype(bool).tolist()
            assert np.array_equal(det_class[b], g["det_class"][b][:g["num_det"][b]])
        return g

    last = run()
    print("ego=%s: %d live tracks, %d with evidence, classes %s at the last scan"
          % (ego, int((last["track_id"] != 0).sum()), int((last["ev_scans"] > 0).sum()),
             np.bincount(last["track_class"].reshape(-1), minlength=4).tolist()))
    assert graphed._graph is not None and eager._graph is None
    for det in (eager, graphed):
        det.reset()
        assert not any(t.any() for t in det._tm_state)
        with pytest.raises(RuntimeError):
            det.track_map()
    again = run()                                              # the same sequence again behind a reset
    for k in FIELDS:
        assert same_bits(again[k], last[k]), k


def test_streaming_detector_constructor_rules():
    from planar_optical_flow_amd.streaming import StreamingDetector
    model = _stream_model(13)
    base = dict(nms_min_dist=0.5, ego_motion=dict(method="keyframe_map"), person_motion=dict())
    for missing in (dict(tracks=dict()), dict(grid_map=dict(size=64)), dict()):
        with pytest.raises(ValueError, match="tracks.*grid_map"):
            StreamingDetector(model, track_map=dict(), **base, **missing)
    full = dict(base, tracks=dict(max_tracks=8), grid_map=dict(size=64))
    for bad in (dict(cap=449), dict(cap=(1 << 20) + 1), dict(free_pct=101), dict(occ_pct=-1), dict(travel=-0.5),
                dict(min_scans=-1), dict(occ_thresh=-1), dict(caps=4096), dict(cls_thresh=0.5)):
        with pytest.raises(ValueError):
            StreamingDetector(model, track_map=bad, **full)
    plain = StreamingDetector(model, **full)
    assert plain._tm_kw is None and not any("_tm_" in name and name != "_tm_kw" for name in dir(plain))
    with pytest.raises(RuntimeError):
        plain.track_map()
    det = StreamingDetector(model, track_map=dict(cap=450, min_scans=1), **full)      # keyframe_map, 8 slots
    assert det._tm_state.ev_id.shape == (1, 8) and det._tm_out.point_class.shape == (1, 450)
    assert det._tm_kw == dict(DEFAULTS, cap=450, min_scans=1)
    for t in range(3):
        det(torch.zeros(450).cuda() + 3.0 + 0.01 * t)
    live, det_class, state, out = det.track_map()
    assert len(live) == 1 and len(det_class[0]) == int(det._dets[2][0]) and out.class_count.sum() == len(live[0])

    class DiffFlow(torch.nn.Module):
        def forward(self, prev, cur):
            return torch.cat([cur - prev, prev - cur], dim=2)

    # with a flow net and a pose per call: the track stage, and this one, run from the second scan on
    flow = StreamingDetector(model, nms_min_dist=0.5, flow_model=DiffFlow(), tracks=dict(), grid_map=dict(size=64),
                             track_map=dict())
    assert [s.from_first for s in flow._stages if s.launch in (flow._track_stage, flow._track_map_stage)] == [False] * 2
    for t in range(3):
        flow(torch.zeros(450).cuda() + 2.0 + 0.01 * t, pose=(0.0, 0.0, 0.0))
    assert flow.track_map()[2] is flow._tm_state
