"""Map-predicted scan (pof_grid_cast, N16) on the GPU: the device against the NumPy restatement of
tests/test_grid_cast.py, every one of the eleven outputs BIT FOR BIT (the float64 fields through an integer view: the
walk calls no libm function, so there is no tolerance and no excluded beam) -- on the rule scenes at their own size and
embedded in scans of 512, 513 and 4096 beams at three placements (the counts launch has one form up to 512 beams and
one beyond), on the rooms of tests/test_grid_map.py and N = 1, 2, 3; at five batch positions, in two runs and in two
replays of a captured launch with a grid update in between; refused calls; through ``utils.OccupancyGrid.cast``; and as
a stage of the streaming detector under two sources of a pose, with and without the scrolling grid, eager and replayed,
against the restated chain."""
import os
import sys

import numpy as np
import pytest
import torch

from test_grid_cast import (DEFAULTS, OUT_DTYPES, OUT_FIELDS, WALL, _cast_case, device_cases, grid_cast_oracle,
                            rule_scenes, run_case, same_bits)
from test_grid_map import DEFAULTS as MAP_DEFAULTS, ambiguous_cells, grid_map_oracle, room_scene
from test_grid_scroll import grid_scroll_oracle

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "planar_optical_flow_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)


@pytest.fixture(scope="module")
def ops():
    from planar_optical_flow_amd import ops as _ops
    return _ops


def _inputs(steps, tab, origins):
    """One step's inputs of B sensors as device tensors: (ranges, tab, rot, trans, state) and the NMS keywords."""
    from planar_optical_flow_amd import ops
    stack = lambda k, dt: torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(s[k]) for s in steps]), dtype=dt)).cuda()
    nms = {}
    if "inst" in steps[0]:
        nms = dict(instance_mask=stack("inst", np.int32), num_det=stack("num_det", np.int32),
                   det_cls=stack("det_cls", np.float64))
    state = ops.GridMapState(stack("grid", np.int16), torch.from_numpy(np.stack(origins).astype(np.float64)).cuda())
    return (stack("ranges", np.float32), torch.from_numpy(np.asarray(tab, np.float64)).cuda(), stack("rot", np.float32),
            stack("trans", np.float64), state), nms


def _host(out):
    return {k: getattr(out, k).cpu().numpy() for k in OUT_FIELDS}


def dev_steps(ops, case, sensors=None):
    """The device's outputs for every step, all sensors of the case in one batch."""
    sensors = case["sensors"] if sensors is None else sensors
    res = []
    for steps in zip(*[s["steps"] for s in sensors]):
        args, nms = _inputs(steps, case["tab"], [s["origin"] for s in sensors])
        before = args[4].grid.clone()
        res.append(_host(ops.grid_cast(*args, res=case["res"], **nms, **case["kw"])))
        assert torch.equal(args[4].grid, before)               # the grid is read only
    return res


def check_case(ops, case, what):
    got = dev_steps(ops, case)
    walls = 0
    for b, sensor in enumerate(case["sensors"]):
        for t, want in enumerate(run_case(case, sensor)):
            for k, dt in zip(OUT_FIELDS, OUT_DTYPES):
                assert got[t][k].dtype == dt and same_bits(got[t][k][b], want[k]), (what, b, t, k)
            walls += int((want["exp_state"] == WALL).sum())
    print("%s: %d sensors x %d steps, %d beams end on a wall, every field the restatement's bits"
          % (what, len(case["sensors"]), len(case["sensors"][0]["steps"]), walls))
    return got


# ------------------------------------------------------------------ 1. the device against the restatement
@pytest.mark.parametrize("name", sorted(rule_scenes()))
def test_rule_scenes(ops, name):
    check_case(ops, rule_scenes()[name], name)


FILL_PAIRS = ((1.0, 0.0), (0.5, 0.5), (-1.0, 0.25), (0.0, -1.0), (-0.5, -0.75), (0.25, 1.0), (0.0, 0.0))
FILL_RANGES = (0.5, 1.0, 2.5, np.inf, 0.9375)


def embedded(case, N, at):
    """The one-step rule scene ``case`` with its n beams at beams at..at + n of a scan of N: around them beams of seven
    dyadic directions and five ranges that are nobody's."""
    step = case["sensors"][0]["steps"][0]
    n = len(step["ranges"])
    tab = np.asarray(case["tab"], np.float64)
    pairs = np.array([FILL_PAIRS[i % len(FILL_PAIRS)] for i in range(N)])
    ranges = np.array([FILL_RANGES[i % len(FILL_RANGES)] for i in range(N)], np.float32)
    pairs[at:at + n], ranges[at:at + n] = tab[n:].reshape(n, 2), step["ranges"]
    big = dict(step, ranges=ranges)
    if "inst" in step:
        inst = np.zeros(N, np.int32)
        inst[at:at + n] = step["inst"]
        big.update(inst=inst, det_cls=np.zeros(N))
    return dict(case, tab=np.concatenate([np.zeros(N), pairs.reshape(-1)]),
                sensors=[dict(case["sensors"][0], steps=[big])])


@pytest.mark.parametrize("N", [512, 513, 4096])
def test_rule_scenes_embedded_in_long_scans(ops, N):
    scenes, beams = rule_scenes(), 0
    for name, case in scenes.items():
        n = len(case["sensors"][0]["steps"][0]["ranges"])
        small = run_case(case, case["sensors"][0])[0]
        for at in (0, (N - n) // 2 + 1, N - n):
            big = embedded(case, N, at)
            got = dev_steps(ops, big)[0]
            want = run_case(big, big["sensors"][0])[0]
            for k in OUT_FIELDS:
                assert same_bits(got[k][0], want[k]), (name, N, at, k)
            for k in OUT_FIELDS[:7]:                           # per beam: the scene's own values, wherever it stands
                assert same_bits(want[k][at:at + n], small[k]), (name, N, at, k)
            beams += N
    print("N = %d: %d scenes at three placements, %d beams, every field the restatement's bits" % (N, len(scenes), beams))


@pytest.mark.parametrize("name", ["rooms", "one tile", "128 x 192", "N 512", "N 513", "N 4096", "no NMS", "2048 x 2048",
                                  "N 1", "N 2", "N 3", "outside", "no rotation"])
def test_room_cases(ops, name):
    got = check_case(ops, device_cases()[name], name)
    if name == "rooms":
        assert (got[-1]["point_class"] == 1).sum() > 500 and got[-1]["det_novel"].any()
    if name == "no NMS":
        assert not any(g[k].any() for g in got for k in ("det_novel", "det_map", "det_through"))


# ------------------------------------------------------------------ 2. determinism
def test_same_bits_at_five_batch_positions_and_in_two_runs(ops):
    case = device_cases()["128 x 192"]
    me, other = case["sensors"][0], _cast_case(room_scene(43, 3, 450, 128, 192))["sensors"][0]     # another room
    want = run_case(case, me)
    runs = []
    for pos in list(range(5)) + [2]:
        sensors = [other] * 5
        sensors[pos] = me
        got = dev_steps(ops, case, sensors)
        for t, w in enumerate(want):
            for k in OUT_FIELDS:
                assert same_bits(got[t][k][pos], w[k]), (pos, t, k)
        runs.append(got)
    for k in OUT_FIELDS:                                       # the two runs at position 2: every sensor's bits
        assert all(same_bits(a[k], b[k]) for a, b in zip(runs[2], runs[5])), k


def test_two_replays_of_a_captured_launch_with_a_grid_update_between_them(ops):
    case = device_cases()["rooms"]
    sensors, scene = case["sensors"], case["map"]
    B, N, T = len(sensors), 450, len(sensors[0]["steps"])
    want = list(zip(*[run_case(case, s) for s in sensors]))    # [t][b]
    origins = [s["origin"] for s in sensors]
    steps = [_inputs(st, case["tab"], origins) for st in zip(*[s["steps"] for s in sensors])]
    args = [t.clone() if i == 1 else torch.zeros_like(t) for i, t in enumerate(steps[0][0][:4])]
    nms = {k: torch.zeros_like(t) for k, t in steps[0][1].items()}
    state = ops.GridMapState(torch.zeros_like(steps[0][0][4].grid), steps[0][0][4].origin.clone())
    out = ops.grid_cast_buffers(B, N)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                              # warm-up into buffers of its own
        ops.grid_cast(*args, state, res=case["res"], **nms, **case["kw"])
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.grid_cast(*args, state, res=case["res"], out=out, **nms, **case["kw"])
    for _ in range(2):
        state.grid.zero_()
        for t in range(T):
            for dst, src in zip(args, steps[t][0][:4]):
                dst.copy_(src)
            for k in nms:
                nms[k].copy_(steps[t][1][k])
            graph.replay()
            got = _host(out)
            for b in range(B):
                for k in OUT_FIELDS:
                    assert same_bits(got[k][b], want[t][b][k]), (t, b, k)
            # the scan enters the grid: the next replay walks another map
            ops.grid_map_update(*args, state, res=scene["res"], **nms, **scene["kw"])
            if t + 1 < T:
                assert torch.equal(state.grid, steps[t + 1][0][4].grid)
    assert want[0][0]["class_count"].tolist() != want[-1][0]["class_count"].tolist()


# ------------------------------------------------------------------ 3. refused calls
def test_refused_calls_leave_the_outputs_untouched(ops):
    from planar_optical_flow_amd import _lib
    from planar_optical_flow_amd._lib import POF_E_SHAPE, PofError
    rng = np.random.default_rng(1)
    base = dict(DEFAULTS, res=0.1)
    cases = ((4097, 64, 64, {}, PofError), (64, 64, 96, {}, PofError), (64, 2112, 64, {}, PofError),
             (64, 64, 64, dict(res=0.0), AssertionError), (64, 64, 64, dict(max_range=0.0), AssertionError),
             (64, 64, 64, dict(tol=-1.0), AssertionError), (64, 64, 64, dict(occ_thresh=0), AssertionError),
             (64, 64, 64, dict(free_thresh=-1), AssertionError), (64, 64, 64, dict(max_range=float("nan")), AssertionError))
    for N, H, W, kw, error in cases:
        scene = room_scene(5, 1, N, 64, 64)
        s = scene["sensors"][0]["scans"][0]
        step = dict(s, grid=rng.integers(-40, 70, (H, W)).astype(np.int16))
        args, nms = _inputs([step], scene["tab"], [scene["sensors"][0]["origin"]])
        out = ops.grid_cast_buffers(1, N)
        for t in out:                                          # sentinels
            t.copy_(torch.from_numpy(rng.integers(1, 100, tuple(t.shape))).to(t.dtype))
        before = [t.cpu().numpy() for t in out] + [args[4].grid.cpu().numpy()]
        with pytest.raises(error) as e:
            ops.grid_cast(*args, out=out, **nms, **dict(base, **kw))
        if error is PofError:
            assert e.value.code == POF_E_SHAPE
        after = [t.cpu().numpy() for t in out] + [args[4].grid.cpu().numpy()]
        assert all(np.array_equal(a, b) for a, b in zip(before, after)), (N, H, W, kw)
    # the NMS results in part: refused by the wrapper and by the entry point itself
    scene = room_scene(5, 1, 64, 64, 64)
    s = scene["sensors"][0]["scans"][0]
    args, nms = _inputs([dict(s, grid=np.full((64, 64), 20, np.int16))], scene["tab"], [scene["sensors"][0]["origin"]])
    out = ops.grid_cast_buffers(1, 64)
    for part in (("instance_mask",), ("num_det", "det_cls"), ("instance_mask", "det_cls")):
        with pytest.raises(ValueError):
            ops.grid_cast(*args, out=out, res=0.1, **{k: nms[k] for k in part})
    ptr = lambda t: t.data_ptr()
    rc = _lib.load().pof_grid_cast(ptr(args[0]), ptr(args[1]), ptr(args[2]), ptr(args[3]), ptr(nms["instance_mask"]), None,
                                   ptr(nms["det_cls"]), ptr(args[4].grid), ptr(args[4].origin), 0.1, 20.0, 0.1, 17, 16, 1,
                                   64, 64, 64, *[ptr(t) for t in out], None)
    torch.cuda.synchronize()
    assert rc == _lib.POF_E_BADARG and not any(t.any() for t in out)
    with pytest.raises(ValueError):
        ops.grid_cast(*args[:4], ops.grid_map_state(2, 64, 64), res=0.1)              # the state of another batch
    with pytest.raises(ValueError):
        ops.grid_cast(*args, res=0.1, out=ops.grid_cast_buffers(1, 65))
    with pytest.raises(ValueError):
        ops.grid_cast(args[0], args[1], args[2], args[3][:, :1], args[4], res=0.1)    # trans [B,1]
    empty = ops.grid_cast(args[0][:0], args[1], args[2][:0], args[3][:0], ops.grid_map_state(0, 64, 64), res=0.1)
    assert empty.exp_range.shape == (0, 64) and empty.class_count.shape == (0, 5)
    # the next good call works: a grid of 20s is a wall in the first cell of every beam
    o = ops.grid_cast(*args, res=0.1, out=out, **nms)
    assert o is out and bool((o.exp_state == WALL).all()) and bool((o.exp_steps >= 2).all())
    want = grid_cast_oracle(s["ranges"], scene["tab"], s["rot"], s["trans"], np.full((64, 64), 20, np.int16),
                            scene["sensors"][0]["origin"], 0.1, s["inst"], s["num_det"], s["det_cls"])
    assert all(same_bits(getattr(o, k)[0].cpu().numpy(), want[k]) for k in OUT_FIELDS)


# ------------------------------------------------------------------ 4. the wrapper and the reference-shaped class
def test_wrapper_with_out_and_occupancy_grid_cast_equal_the_direct_call(ops):
    import src.utils.utils as u
    from test_person_motion import people_scene
    scene = people_scene(24, 4, 0.2)
    N, res, size = 450, 0.1, (128, 192)
    phi = scene["tab"][:N]
    rng = np.random.default_rng(3)
    og = u.OccupancyGrid(phi, res=res, size=size, max_range=10.0, min_dist=0.5)
    tab = u._table_for(phi)
    state = ops.grid_map_state(1, *size)
    ops.grid_map_reset(state, scene["poses"][0][:2] - 0.5 * res * np.array([192.0, 128.0]))
    out = ops.grid_cast_buffers(1, N)
    cls, reg = rng.uniform(0.05, 0.95, (N, 1)), rng.normal(0.0, 0.05, (N, 2))
    for t, s in enumerate(scene["scans"]):
        gated = t != 1                                         # one scan without predictions
        preds = (cls, reg) if gated else ()
        got = og.cast(s["ranges"], scene["poses"][t], *preds, tol=0.15)       # before the scan's update
        og.update(s["ranges"], scene["poses"][t], *preds)
        ranges = torch.from_numpy(s["ranges"]).cuda().reshape(1, N)
        nms = {}
        if gated:
            _, dc, num, inst = ops.nms_predicted_center(ranges, tab, torch.from_numpy(cls[:, 0].copy()).cuda().reshape(1, N),
                                                        torch.from_numpy(reg).cuda().reshape(1, N, 2), 0.5)
            nms = dict(instance_mask=inst, num_det=num, det_cls=dc)
        rot, trans, _ = u._pose_terms(scene["poses"][t][None])
        pose = (torch.from_numpy(rot).cuda(), torch.from_numpy(trans).cuda())
        fresh = ops.grid_cast(ranges, tab, *pose, state, res=res, max_range=10.0, tol=0.15, **nms)
        o = ops.grid_cast(ranges, tab, *pose, state, res=res, max_range=10.0, tol=0.15, out=out, **nms)
        assert o is out and type(fresh) is ops.GridCast
        for a, b in zip(fresh, o):
            assert a.data_ptr() != b.data_ptr() and same_bits(a.cpu().numpy(), b.cpu().numpy())
        # against the restatement too, with the table the device made (its cosines and sines are the device's own)
        want = grid_cast_oracle(s["ranges"], tab.cpu().numpy(), rot[0], trans[0], state.grid[0].cpu().numpy(),
                                state.origin[0].cpu().numpy(), res, *[v[0].cpu().numpy() for v in nms.values()],
                                max_range=10.0, tol=0.15)
        m = int(nms["num_det"][0]) if gated else 0
        for k in OUT_FIELDS:
            assert same_bits(getattr(o, k)[0].cpu().numpy(), want[k]), (t, k)
            if not k.startswith("det_"):
                assert same_bits(got[k], want[k]), (t, k)
            elif gated:
                assert np.array_equal(got[k], want[k][:m]), (t, k)
            else:
                assert k not in got
        assert ("instance_mask" in got) == gated
        ops.grid_map_update(ranges, tab, *pose, state, res=res, max_range=10.0, **nms)
        assert np.array_equal(og.logodds, state.grid[0].cpu().numpy()) and np.array_equal(og.origin, state.origin[0].cpu().numpy())
    assert (want["point_class"] == 1).sum() > 100              # by the last scan the walls are in the map
    with pytest.raises(ValueError, match="unknown grid_cast settings"):
        og.cast(scene["scans"][0]["ranges"], scene["poses"][0], max_range=5.0)    # the grid's own
    fresh_grid = u.OccupancyGrid(phi, res=res, size=64)
    first = fresh_grid.cast(scene["scans"][0]["ranges"], (1.0, 2.0, 0.5))           # centres the grid as update would
    assert fresh_grid.origin.tolist() == [1.0 - 3.2, 2.0 - 3.2] and not (first["exp_state"] == 4).any()
    fresh_grid.update(scene["scans"][0]["ranges"], (1.0, 2.0, 0.5))
    assert fresh_grid.origin.tolist() == [1.0 - 3.2, 2.0 - 3.2]


# ------------------------------------------------------------------ 5. streaming detector
STREAM_T, STREAM_SIZE, STREAM_RES, STREAM_RANGE = 12, 192, 0.05, 6.0


def _stream_model(seed):
    from planar_optical_flow_amd.src.depracted.model.dr_spaam import SpatialDROW
    torch.manual_seed(seed)
    return SpatialDROW(num_scans=5, num_pts=56, alpha=0.5, window_size=11, pedestrian_only=True).cuda().eval()


def _snapshot(det, scroll):
    """Everything the cast, the scroll and the grid stage read and leave behind, on the host."""
    _, conf, num, inst = det._dets
    state, _ = det.grid_map()
    snap = {"pred_cls": det.pred_cls, "det_cls": conf, "num_det": num, "inst": inst, "rot": det._pose_rot,
            "trans": det._pose_trans, "grid": state.grid, "origin": state.origin}
    snap.update(zip(OUT_FIELDS, det.grid_cast()))
    if scroll:
        snap.update(shift=det._gs_out.shift, offset=det._gs_state.offset)
        if det._sg_kw is not None:
            snap.update(moved=det._sg_out.moved, correction=det._sg_out.correction)
    return {k: v.detach().cpu().numpy().copy() for k, v in snap.items()}


@pytest.mark.parametrize("scroll", [False, True])
@pytest.mark.parametrize("ego", ["keyframe", "scan_match"])
def test_streaming_detector_eager_graph_and_restated_chain(ego, scroll):
    from planar_optical_flow_amd.streaming import StreamingDetector
    from test_grid_scroll_gpu import two_drives
    B, size, res = 2, STREAM_SIZE, STREAM_RES
    T = STREAM_T if scroll else 6                              # the drives scroll around scans 8 and 10
    scans, poses = two_drives()
    model = _stream_model(13)
    cast_kw = dict(max_range=STREAM_RANGE, tol=0.075)
    kw = dict(batch=B, nms_min_dist=0.5, cls_thresh=0.5, grid_map=dict(size=size, res=res, max_range=STREAM_RANGE),
              ego_motion=dict(method=ego))
    if scroll:
        kw["grid_scroll"] = dict(margin=64)
        if ego == "scan_match":
            kw["grid_match"] = dict(max_range=STREAM_RANGE)
    eager = StreamingDetector(model, graph=False, grid_cast=cast_kw, **kw)
    graphed = StreamingDetector(model, graph=True, grid_cast=cast_kw, **kw)
    parent = StreamingDetector(model, graph=True, **kw)         # what the detector is without the stage
    assert parent._gc_kw is None and not hasattr(parent, "_gc_out") and len(eager._stages) == len(parent._stages) + 1
    names = [s.launch.__name__ for s in graphed._stages]
    assert names.index("_grid_cast_stage") == names.index("_grid_stage") - 1       # directly in front of the grid map
    assert all(names.index(n) < names.index("_grid_cast_stage") for n in names if n in ("_grid_scroll_stage",
                                                                                         "_grid_match_stage"))
    tab = graphed.tab.cpu().numpy()
    settings = dict(MAP_DEFAULTS, max_range=STREAM_RANGE)
    half = 0.5 * res * size
    start = poses[0][:, :2]

    def run():
        grids = [np.zeros((size, size), np.int16) for _ in range(B)]
        origins, offsets = [start[b] - half for b in range(B)], [np.zeros(2, np.int32) for _ in range(B)]
        classes, scrolled = np.zeros(5, np.int64), 0
        for det in (eager, graphed, parent):
            det.reset(pose=poses[0])
        for t in range(T):
            for det in (eager, graphed, parent):
                if t == 0 and det is not parent:
                    with pytest.raises(RuntimeError, match="grid_cast"):
                        det.grid_cast()
                det(torch.from_numpy(scans[t]).cuda())
            e, g = _snapshot(eager, scroll), _snapshot(graphed, scroll)
            for k in e:
                assert same_bits(e[k], g[k]), (t, k)           # eager and replayed: identical bits
            # the stage reads and writes nothing of the others: the grid is the parent's
            assert torch.equal(parent._gm_state.grid, graphed._gm_state.grid) and \
                torch.equal(parent._gm_out.point_prior, graphed._gm_out.point_prior)
            for b in range(B):
                if scroll:
                    trans = g["trans"][b] - g["correction"][b, :2] if "moved" in g and g["moved"][b] else g["trans"][b]
                    s = grid_scroll_oracle(trans, grids[b], origins[b], start[b] - half, offsets[b], res, 64)
                    assert np.array_equal(g["shift"][b], s["shift"]), (t, b)
                    scrolled += int(s["scrolled"])
                assert g["origin"][b].tobytes() == origins[b].tobytes(), (t, b)
                want = grid_cast_oracle(scans[t, b], tab, g["rot"][b], g["trans"][b], grids[b], origins[b], res,
                                        g["inst"][b], g["num_det"][b], g["det_cls"][b], **dict(DEFAULTS, **cast_kw))
                for k in OUT_FIELDS:
                    assert same_bits(g[k][b], want[k]), (t, b, k)
                classes += want["class_count"]
                if t == 0:                                     # an empty map: every beam runs out of it or of range
                    assert not (want["exp_state"] == WALL).any() and not want["class_count"][[1, 2, 3]].any()
                assert ambiguous_cells(tab, g["rot"][b], g["trans"][b], origins[b], res, size, size, STREAM_RANGE) == 0
                grid_map_oracle(scans[t, b], tab, g["rot"][b], g["trans"][b], grids[b], origins[b], res, g["inst"][b],
                                g["num_det"][b], g["det_cls"][b], **settings)
                assert np.array_equal(g["grid"][b], grids[b]), (t, b)
        assert graphed.grid_cast() is graphed._gc_out and type(graphed._gc_out).__name__ == "GridCast"
        return classes, scrolled

    classes, scrolled = run()
    print("ego=%s scroll=%s: points per class over %d scans of %d sensors %s, %d scrolls"
          % (ego, scroll, T, B, classes.tolist(), scrolled))
    assert classes[1] > 1000 and classes[4] > 0 and (scrolled >= 2) == scroll
    assert graphed._graph is not None and eager._graph is None
    for det in (eager, graphed):
        det.reset(pose=(1.0, -2.0, 0.25))
        with pytest.raises(RuntimeError):
            det.grid_cast()
    again = run()                                              # the same sequence again behind a reset
    assert np.array_equal(again[0], classes) and again[1] == scrolled


def test_streaming_detector_constructor_rules():
    from planar_optical_flow_amd.streaming import StreamingDetector
    model = _stream_model(13)
    with pytest.raises(ValueError, match="grid_map"):
        StreamingDetector(model, grid_cast=dict())
    with pytest.raises(ValueError, match="grid_map"):
        StreamingDetector(model, nms_min_dist=0.5, ego_motion=dict(method="keyframe"), grid_cast=dict())
    for bad in (dict(max_range=0.0), dict(tol=-0.1), dict(occ_thresh=0), dict(free_thresh=-1)):
        with pytest.raises(ValueError, match="grid_cast"):
            StreamingDetector(model, grid_map=dict(size=64), grid_cast=bad)
    for bad in (dict(res=0.1), dict(cls_thresh=0.5), dict(tols=1.0)):
        with pytest.raises(ValueError, match="unknown grid_cast settings"):
            StreamingDetector(model, grid_map=dict(size=64), grid_cast=bad)
    plain = StreamingDetector(model, grid_map=dict(size=64))
    assert plain._gc_kw is None and not any(name.startswith("_gc_") and name != "_gc_kw" for name in dir(plain))
    with pytest.raises(RuntimeError, match="grid_cast"):
        plain.grid_cast()
    # a pose per call and no NMS: the cast runs from the first scan, on an empty map, and the second scan finds the first
    cast = StreamingDetector(model, grid_map=dict(size=(64, 128), res=0.125), grid_cast=dict(occ_thresh=10))
    assert cast._gc_kw == dict(max_range=20.0, tol=None, occ_thresh=10, free_thresh=16)
    with pytest.raises(RuntimeError, match="grid_cast"):
        cast.grid_cast()
    scan = torch.zeros(450).cuda() + 3.0
    cast(scan, pose=(1.0, 2.0, 0.5))
    o = cast.grid_cast()
    assert o is cast._gc_out and not bool((o.exp_state == WALL).any()) and not o.det_map.any()
    assert o.class_count.cpu().numpy().tolist() == [[0, 0, 0, 0, 450]]
    cast(scan, pose=(1.0, 2.0, 0.5))
    o = cast.grid_cast()
    seen = cast.grid_map()[1]
    own = (seen.point_prior >= 10) & (o.exp_cell == seen.point_cell)           # the first occupied cell is the beam's own
    assert int(own.sum()) > 100 and bool((o.point_class[own] == 1).all()) and not bool((o.point_class == 2).any())
