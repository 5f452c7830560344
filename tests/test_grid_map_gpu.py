"""Occupancy grid map (pof_grid_map_update, N12) on the GPU: the device against the NumPy restatement of
tests/test_grid_map.py with the grid carried on the device, the grid and the five outputs BIT FOR BIT after every scan
(integers throughout; the one transcendental, the atan2 of the cell rule, only picks a beam, and tests/test_grid_map.py
asserts that no cell of these scenes is within 1e-9 of the boundary between two beams, so there is no tolerance and no
excluded cell) -- on rooms with people, at both forms of the points launch, one tile, H != W, the longest scan and the
largest grid, on the rule scenes; at five batch positions, in two runs and in two replays of a captured step; refused
calls; through ``utils.OccupancyGrid``; and as a stage of the streaming detector with the three sources of a pose, eager
and replayed."""
import os
import sys

import numpy as np
import pytest
import torch

from test_grid_map import (DEFAULTS, OUT_DTYPES, OUT_FIELDS, ambiguous_cells, device_scenes, grid_map_oracle,
                           room_scene, rule_scenes, run_sensor)
from test_scan_match import trajectory

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "planar_optical_flow_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

FIELDS = OUT_FIELDS + ("grid",)


@pytest.fixture(scope="module")
def ops():
    from planar_optical_flow_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def scenes():
    return device_scenes()


def _inputs(scans, tab):
    """One step's inputs of B sensors as device tensors: (ranges, tab, rot, trans) and the NMS keywords."""
    stack = lambda k, dt: torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(s[k]) for s in scans]), dtype=dt)).cuda()
    nms = {}
    if "inst" in scans[0]:
        nms = dict(instance_mask=stack("inst", np.int32), num_det=stack("num_det", np.int32),
                   det_cls=stack("det_cls", np.float64))
    return (stack("ranges", np.float32), torch.from_numpy(np.asarray(tab, np.float64)).cuda(), stack("rot", np.float32),
            stack("trans", np.float64)), nms


def _state(ops, scene, sensors):
    state = ops.grid_map_state(len(sensors), scene["H"], scene["W"])
    ops.grid_map_reset(state, torch.from_numpy(np.stack([s["origin"] for s in sensors])).cuda())
    return state


def _host(out, state):
    h = {k: getattr(out, k).cpu().numpy() for k in OUT_FIELDS}
    h["grid"] = state.grid.cpu().numpy()
    return h


def dev_steps(ops, scene, sensors=None):
    """The device's outputs and grid after every scan, all sensors of the scene in one batch."""
    sensors = scene["sensors"] if sensors is None else sensors
    N = len(sensors[0]["scans"][0]["ranges"])
    state, out, res = _state(ops, scene, sensors), ops.grid_map_buffers(len(sensors), N), []
    for scans in zip(*[s["scans"] for s in sensors]):
        args, nms = _inputs(scans, scene["tab"])
        ops.grid_map_update(*args, state, res=scene["res"], out=out, **nms, **scene["kw"])
        res.append(_host(out, state))
    return res


def check_scene(ops, scene, what):
    got = dev_steps(ops, scene)
    cells = 0
    for b, sensor in enumerate(scene["sensors"]):
        for t, want in enumerate(run_sensor(scene, sensor)):
            for k, dt in zip(FIELDS, OUT_DTYPES + (np.int16,)):
                assert got[t][k].dtype == dt and np.array_equal(got[t][k][b], want[k]), (what, b, t, k)
            cells += int((want["grid"] != 0).sum())
    print("%s: %d sensors x %d scans, %d known cells in all, every field the restatement's bits"
          % (what, len(scene["sensors"]), len(scene["sensors"][0]["scans"]), cells))
    return got


# ------------------------------------------------------------------ 1. the device against the restatement
def test_rooms_with_people_every_scan(ops, scenes):
    got = check_scene(ops, scenes["rooms"], "rooms")
    last = got[-1]
    assert (last["grid"] > 0).any() and (last["grid"] < 0).any() and last["det_free"].any()


@pytest.mark.parametrize("name", ["one tile", "128 x 192", "N 512", "N 513", "N 4096", "no NMS", "2048 x 2048"])
def test_shapes(ops, scenes, name):
    got = check_scene(ops, scenes[name], name)
    assert got[-1]["grid"].any()
    if name == "no NMS":
        assert not got[-1]["det_points"].any() and not got[-1]["det_free"].any()


@pytest.mark.parametrize("name", sorted(rule_scenes()))
def test_rule_scenes(ops, name):
    check_scene(ops, rule_scenes()[name], name)


def test_cells_without_a_change_keep_their_bits(ops):
    scene = rule_scenes()["base"]
    sensor = scene["sensors"][0]
    state, s = _state(ops, scene, [sensor]), sensor["scans"][0]
    state.grid.fill_(99)                                       # outside [lo, hi]
    want = np.full((scene["H"], scene["W"]), 99, np.int16)
    grid_map_oracle(s["ranges"], scene["tab"], s["rot"], s["trans"], want, sensor["origin"], scene["res"], **scene["kw"])
    args, nms = _inputs([s], scene["tab"])
    ops.grid_map_update(*args, state, res=scene["res"], **nms, **scene["kw"])
    got = state.grid[0].cpu().numpy()
    assert np.array_equal(got, want) and (got == 99).sum() > 7000 and (got == 70).any()


# ------------------------------------------------------------------ 2. determinism
def test_same_bits_at_five_batch_positions_and_in_two_runs(ops, scenes):
    scene = scenes["128 x 192"]
    me, other = scene["sensors"][0], room_scene(43, 3, 450, 128, 192)["sensors"][0]
    want = run_sensor(scene, me)
    runs = []
    for pos in list(range(5)) + [2]:
        sensors = [other] * 5
        sensors[pos] = me
        got = dev_steps(ops, scene, sensors)
        for t, w in enumerate(want):
            for k in FIELDS:
                assert np.array_equal(got[t][k][pos], w[k]), (pos, t, k)
        runs.append(got)
    for k in FIELDS:                                           # the two runs at position 2: every sensor's bits
        assert all(np.array_equal(a[k], b[k]) for a, b in zip(runs[2], runs[5])), k


def test_two_replays_of_a_captured_step_with_a_reset_in_between(ops, scenes):
    scene = scenes["rooms"]
    sensors = scene["sensors"]
    B, N, T = len(sensors), 450, len(sensors[0]["scans"])
    want = dev_steps(ops, scene)
    steps = [_inputs(scans, scene["tab"]) for scans in zip(*[s["scans"] for s in sensors])]
    args = [torch.zeros_like(t) for t in steps[0][0]]
    nms = {k: torch.zeros_like(t) for k, t in steps[0][1].items()}
    args[1].copy_(steps[0][0][1])                              # the table
    state, out = _state(ops, scene, sensors), ops.grid_map_buffers(B, N)
    origin = state.origin.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                              # warm-up on a state of its own
        ops.grid_map_update(*args, _state(ops, scene, sensors), res=scene["res"], **nms, **scene["kw"])
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.grid_map_update(*args, state, res=scene["res"], out=out, **nms, **scene["kw"])
    for _ in range(2):
        ops.grid_map_reset(state, origin)
        assert not state.grid.any()
        for t in range(T):
            for dst, src in zip(args, steps[t][0]):
                dst.copy_(src)
            for k in nms:
                nms[k].copy_(steps[t][1][k])
            graph.replay()
            got = _host(out, state)
            for k in FIELDS:
                assert np.array_equal(got[k], want[t][k]), (t, k)


# ------------------------------------------------------------------ 3. refused calls
def test_refused_calls_leave_state_and_outputs_untouched(ops):
    from planar_optical_flow_amd._lib import POF_E_SHAPE, PofError
    rng = np.random.default_rng(1)
    base = dict(DEFAULTS, res=0.1)
    cases = ((4097, 64, 64, {}, PofError), (64, 64, 96, {}, PofError), (64, 2112, 64, {}, PofError),
             (64, 64, 64, dict(res=0.0), AssertionError), (64, 64, 64, dict(hit=-1), AssertionError),
             (64, 64, 64, dict(lo=1), AssertionError), (64, 64, 64, dict(tol=-1.0), AssertionError),
             (64, 64, 64, dict(max_range=0.0), AssertionError), (64, 64, 64, dict(hi=40000), AssertionError),
             (64, 64, 64, dict(free_thresh=-1), AssertionError), (64, 64, 64, dict(miss=-1), AssertionError))
    for N, H, W, kw, error in cases:
        scene = room_scene(5, 1, N, 64, 64)
        s = scene["sensors"][0]["scans"][0]
        state, out = ops.grid_map_state(1, H, W), ops.grid_map_buffers(1, N)
        for t in tuple(state) + tuple(out):                    # sentinels
            t.copy_(torch.from_numpy(rng.integers(1, 100, tuple(t.shape))).to(t.dtype))
        before = [t.cpu().numpy() for t in tuple(state) + tuple(out)]
        args, nms = _inputs([s], scene["tab"])
        with pytest.raises(error) as e:
            ops.grid_map_update(*args, state, out=out, **nms, **dict(base, **kw))
        if error is PofError:
            assert e.value.code == POF_E_SHAPE
        after = [t.cpu().numpy() for t in tuple(state) + tuple(out)]
        assert all(np.array_equal(a, b) for a, b in zip(before, after)), (N, H, W, kw)
    # the NMS results in part: refused by the wrapper and by the entry point itself
    from planar_optical_flow_amd import _lib
    scene = room_scene(5, 1, 64, 64, 64)
    s = scene["sensors"][0]["scans"][0]
    args, nms = _inputs([s], scene["tab"])
    state, out = ops.grid_map_state(1, 64, 64), ops.grid_map_buffers(1, 64)
    state.grid.fill_(7)
    for part in (("instance_mask",), ("num_det", "det_cls"), ("instance_mask", "det_cls")):
        with pytest.raises(ValueError):
            ops.grid_map_update(*args, state, out=out, res=0.1, **{k: nms[k] for k in part})
    ptr = lambda t: t.data_ptr()
    rc = _lib.load().pof_grid_map_update(ptr(args[0]), ptr(args[1]), ptr(args[2]), ptr(args[3]), ptr(nms["instance_mask"]),
                                         None, ptr(nms["det_cls"]), 0.1, 0.1, 20.0, 0.5, 17, 8, -40, 70, 16, 1, 64, 64, 64,
                                         ptr(state.grid), ptr(state.origin), *[ptr(t) for t in out], None)
    torch.cuda.synchronize()
    assert rc == _lib.POF_E_BADARG and bool((state.grid == 7).all()) and not any(t.any() for t in out)
    with pytest.raises(ValueError):
        ops.grid_map_update(*args, ops.grid_map_state(2, 64, 64), res=0.1)                # the state of another batch
    with pytest.raises(ValueError):
        ops.grid_map_update(*args, state, res=0.1, out=ops.grid_map_buffers(1, 65))
    empty = ops.grid_map_update(args[0][:0], args[1], args[2][:0], args[3][:0], ops.grid_map_state(0, 64, 64), res=0.1)
    assert empty.point_cell.shape == (0, 64)
    # the next good call works, and a reset empties the grid
    state = ops.grid_map_state(1, 64, 64)
    ops.grid_map_reset(state, scene["sensors"][0]["origin"])
    o = ops.grid_map_update(*args, state, res=0.1, **nms)
    want = run_sensor(scene, scene["sensors"][0])[0]
    assert np.array_equal(state.grid[0].cpu().numpy(), want["grid"]) and want["grid"].any()
    assert np.array_equal(o.point_cell[0].cpu().numpy(), want["point_cell"])
    ops.grid_map_reset(state)
    assert not state.grid.any() and not state.origin.any()


# ------------------------------------------------------------------ 4. the reference-shaped wrapper
def test_occupancy_grid_wrapper_equals_the_direct_calls(ops):
    import src.utils.utils as u
    from test_person_motion import people_scene
    scene = people_scene(24, 3, 0.2)
    N, res, size = 450, 0.1, (128, 192)
    phi = scene["tab"][:N]
    rng = np.random.default_rng(3)
    og = u.OccupancyGrid(phi, res=res, size=size, max_range=10.0, min_dist=0.5)
    tab = u._table_for(phi)
    state = ops.grid_map_state(1, *size)
    ops.grid_map_reset(state, scene["poses"][0][:2] - 0.5 * res * np.array([192.0, 128.0]))   # the first pose in the middle
    cls, reg = rng.uniform(0.05, 0.95, (N, 1)), rng.normal(0.0, 0.05, (N, 2))
    for t, s in enumerate(scene["scans"]):
        gated = t != 1                                         # one scan without predictions
        got = og.update(s["ranges"], scene["poses"][t], *((cls, reg) if gated else ()))
        ranges = torch.from_numpy(s["ranges"]).cuda().reshape(1, N)
        nms = {}
        if gated:
            _, dc, num, inst = ops.nms_predicted_center(ranges, tab, torch.from_numpy(cls[:, 0].copy()).cuda().reshape(1, N),
                                                        torch.from_numpy(reg).cuda().reshape(1, N, 2), 0.5)
            nms = dict(instance_mask=inst, num_det=num, det_cls=dc)
        rot, trans, _ = u._pose_terms(scene["poses"][t][None])
        o = ops.grid_map_update(ranges, tab, torch.from_numpy(rot).cuda(), torch.from_numpy(trans).cuda(), state, res=res,
                                max_range=10.0, **nms)
        for k in ("point_cell", "point_prior"):
            assert np.array_equal(got[k], getattr(o, k)[0].cpu().numpy()), (t, k)
        assert np.array_equal(got["point_mark"], o.point_mark[0].cpu().numpy().astype(bool)) and got["point_mark"].dtype == bool
        if gated:
            m = int(num[0])
            assert np.array_equal(got["det_points"], o.det_points[0, :m].cpu().numpy()) and len(got["det_free"]) == m
            assert np.array_equal(got["instance_mask"], inst[0].cpu().numpy()) and got["dets_cls"].shape == (m, 1)
        else:
            assert "det_points" not in got
        assert np.array_equal(og.logodds, state.grid[0].cpu().numpy()) and np.array_equal(og.origin, state.origin[0].cpu().numpy())
    p = og.probability()
    assert og.logodds.any() and p.shape == size and p[og.logodds == 0].tolist() == [0.5] * int((og.logodds == 0).sum())
    assert (p[og.logodds > 0] > 0.5).all() and (p[og.logodds < 0] < 0.5).all()
    og.reset((1.0, 2.0))
    assert not og.logodds.any() and og.origin.tolist() == [1.0, 2.0]
    og.update(scene["scans"][0]["ranges"], scene["poses"][0])
    assert og.origin.tolist() == [1.0, 2.0]                    # an origin that was given stays
    og.reset()
    og.update(scene["scans"][0]["ranges"])                     # no pose: the world origin in the middle
    assert og.origin.tolist() == [-0.5 * res * 192, -0.5 * res * 128]
    with pytest.raises(ValueError):
        u.OccupancyGrid(phi, sizes=64)


# ------------------------------------------------------------------ 5. streaming detector
def _stream_model(seed):
    from planar_optical_flow_amd.src.depracted.model.dr_spaam import SpatialDROW
    torch.manual_seed(seed)
    return SpatialDROW(num_scans=5, num_pts=56, alpha=0.5, window_size=11, pedestrian_only=True).cuda().eval()


def _snapshot(det):
    """Everything the grid stage reads and leaves behind, on the host."""
    _, conf, num, inst = det._dets
    state, out = det.grid_map()
    snap = {"pred_cls": det.pred_cls, "det_cls": conf, "num_det": num, "inst": inst, "rot": det._pose_rot,
            "trans": det._pose_trans, "grid": state.grid, "origin": state.origin}
    snap.update({k: getattr(out, k) for k in OUT_FIELDS})
    return {k: v.detach().cpu().numpy().copy() for k, v in snap.items()}


@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("ego", ["keyframe", "scan_match", None])
def test_streaming_detector_eager_graph_and_restatement(ego, tail):
    from planar_optical_flow_amd.streaming import StreamingDetector
    B, T, N, size, res = 2, 6, 450, 128, 0.1
    scans, poses = trajectory(T, B, seed=71, noise=0.01)
    model = _stream_model(13)
    kw = dict(batch=B, nms_min_dist=0.5, cls_thresh=0.5, grid_map=dict(size=size, max_range=6.0))
    if tail:
        kw.update(person_motion=dict(), tracks=dict())
    if ego is not None:
        kw["ego_motion"] = dict(method=ego)
    eager, graphed = StreamingDetector(model, graph=False, **kw), StreamingDetector(model, graph=True, **kw)
    tab = graphed.tab.cpu().numpy()
    settings = dict(DEFAULTS, max_range=6.0)
    half = 0.5 * res * size
    # A dead-reckoning detector starts where reset() puts it.  Not at the world origin: with the 450-beam table the
    # boundary between two beams lies exactly on the diagonals, and a grid that is symmetric about the sensor has cell
    # centres exactly there -- the one place where the last bit of an atan2 decides (asserted for every step below).
    begin = (0.213, -0.127, 0.3)

    def run():
        grids, marked = [np.zeros((size, size), np.int16) for _ in range(B)], 0
        if ego is not None:
            for det in (eager, graphed):
                det.reset(pose=begin)
        for t in range(T):
            for det in (eager, graphed):
                if t == 0:
                    with pytest.raises(RuntimeError):
                        det.grid_map()
                det(torch.from_numpy(scans[t]).cuda(), **({} if ego is not None else dict(pose=poses[t])))
            e, g = _snapshot(eager), _snapshot(graphed)
            for k in e:
                assert np.array_equal(e[k], g[k]), (t, k)      # eager and replayed: identical bits, grid included
            for b in range(B):
                assert ambiguous_cells(tab, g["rot"][b], g["trans"][b], g["origin"][b], res, size, size, 6.0) == 0
                want = grid_map_oracle(scans[t, b], tab, g["rot"][b], g["trans"][b], grids[b], g["origin"][b], res,
                                       g["inst"][b], g["num_det"][b], g["det_cls"][b], **settings)
                for k in OUT_FIELDS:
                    assert np.array_equal(g[k][b], want[k]), (t, b, k)
                assert np.array_equal(g["grid"][b], grids[b]), (t, b)
                marked += int(want["point_mark"].sum())
            start = poses[0][:, :2] if ego is None else np.tile(begin[:2], (B, 1))
            assert np.array_equal(g["origin"], start - half)   # the start pose in the middle of the grid
        return marked, [gr.copy() for gr in grids]

    marked, grids = run()
    print("ego=%s tail=%s: %d marked points over %d scans of %d sensors, %d known cells"
          % (ego, tail, marked, T, B, sum(int((g != 0).sum()) for g in grids)))
    assert marked > 1000 and all((g > 0).any() and (g < 0).any() for g in grids)
    assert graphed._graph is not None and eager._graph is None
    for det in (eager, graphed):
        if ego is None:
            det.reset()
        else:
            det.reset(pose=(1.0, -2.0, 0.25))
            assert np.array_equal(det._gm_state.origin.cpu().numpy(), np.tile([1.0 - half, -2.0 - half], (B, 1)))
        assert not det._gm_state.grid.any()
        with pytest.raises(RuntimeError):
            det.grid_map()
    again = run()                                              # the same sequence again from an empty grid
    assert again[0] == marked and all(np.array_equal(a, b) for a, b in zip(again[1], grids))


def test_streaming_detector_constructor_rules():
    from planar_optical_flow_amd.streaming import StreamingDetector
    model = _stream_model(13)

    class DiffFlow(torch.nn.Module):
        def forward(self, prev, cur):
            return torch.cat([cur - prev, prev - cur], dim=2)

    with pytest.raises(ValueError):                            # method="flow" is not built
        StreamingDetector(model, nms_min_dist=0.5, flow_model=DiffFlow(), ego_motion=dict(), grid_map=dict())
    for bad in (dict(size=96), dict(size=4096), dict(size=(64, 64, 64)), dict(res=0.0), dict(sizes=64)):
        with pytest.raises(ValueError):
            StreamingDetector(model, grid_map=bad)
    plain = StreamingDetector(model, nms_min_dist=0.5)
    assert plain._gm_kw is None
    assert not any(("_gm_" in name or "grid" in name) and not callable(getattr(plain, name)) and name != "_gm_kw"
                   for name in dir(plain))                     # none of the new buffers
    with pytest.raises(RuntimeError):
        plain.grid_map()
    with pytest.raises(ValueError):
        plain(torch.zeros(450).cuda() + 5.0, pose=(0.0, 0.0, 0.0))
    matched = StreamingDetector(model, ego_motion=dict(method="scan_match"))
    assert not hasattr(matched, "_pm_no_ok") and not hasattr(matched, "_pose_dev") and not hasattr(matched, "_gm_state")
    # no NMS: nobody is gated, the map still runs; a pose per call, (H, W) sizes
    mapped = StreamingDetector(model, grid_map=dict(size=(64, 128), res=0.125, hit=5))
    assert mapped._gm_state.grid.shape == (1, 64, 128) and mapped._gm_kw["hit"] == 5 and not hasattr(mapped, "_pm_out")
    mapped(torch.zeros(450).cuda() + 3.0, pose=(1.0, 2.0, 0.5))
    state, out = mapped.grid_map()
    assert state is mapped._gm_state and out is mapped._gm_out
    assert state.origin.cpu().numpy().tolist() == [[1.0 - 8.0, 2.0 - 4.0]]
    assert int((state.grid == 5).sum()) > 20 and int((state.grid == -8).sum()) > 500 and not out.det_points.any()
    assert bool(out.point_mark.all())
    with pytest.raises(ValueError):
        StreamingDetector(model, ego_motion=dict(method="keyframe"), grid_map=dict(size=64))(
            torch.zeros(450).cuda() + 5.0, pose=(0.0, 0.0, 0.0))                  # a dead-reckoning detector takes no pose
    with_flow = StreamingDetector(model, nms_min_dist=0.5, flow_model=DiffFlow(), grid_map=dict(size=64))
    for t in range(3):
        with_flow(torch.zeros(450).cuda() + 2.0 + 0.01 * t, pose=(0.0, 0.0, 0.0))
    assert with_flow.grid_map()[0].grid.any() and with_flow.person_flow()[1] is with_flow._pf_out
