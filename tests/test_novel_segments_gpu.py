"""Novelty segments (pof_novel_segments, N17) on the GPU: the device against the NumPy restatement of
tests/test_novel_segments.py, every one of the ten outputs BIT FOR BIT (the float64 fields through an integer view: the
stage calls no libm function, so there is no tolerance) -- on the rule scenes at their own size and embedded at the
start, the middle and the end of scans of 512, 513 and 4096 beams (one wave up to 512 beams, 512 threads beyond), on the
class-byte patterns, on the rooms of tests/test_grid_cast.py cast by the device itself; at five batch positions, in two
runs and in two replays of a captured launch; refused calls; through ``utils.OccupancyGrid.novel_segments``; the record
as the input of ``ops.person_motion`` and ``ops.track_update``; and as a stage of the streaming detector under two
sources of a pose with the scrolling grid, eager and replayed, against the restated chain, with and without the segments
as the grid map's gate."""
import os
import sys

import numpy as np
import pytest
import torch

from test_grid_cast import DEFAULTS as CAST_DEFAULTS, device_cases as cast_device_cases, grid_cast_oracle
from test_grid_map import DEFAULTS as MAP_DEFAULTS, grid_map_oracle
from test_grid_scroll import grid_scroll_oracle
from test_novel_segments import (DEFAULTS, OTHER_BYTES, OUT_DTYPES, OUT_FIELDS, novel_segments_oracle, pattern_cases,
                                 rule_scenes, run_case, same_bits)
from test_person_motion import motion_state, people_scene, person_motion_oracle, same_bits as same_bits_nan
from test_tracks import FLOAT_FIELDS as TRACK_FLOAT, INT_FIELDS as TRACK_INT, new_state as new_track_state, track_step

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "planar_optical_flow_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)


@pytest.fixture(scope="module")
def ops():
    from planar_optical_flow_amd import ops as _ops
    return _ops


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def _inputs(cases):
    """B cases of one N and one table as device tensors: (ranges, tab, point_class) and the NMS keywords."""
    stack = lambda k, dt: _dev(np.stack([np.asarray(c[k]) for c in cases]), dt)
    nms = {}
    if "inst" in cases[0]:
        nms = dict(instance_mask=stack("inst", np.int32), num_det=stack("num_det", np.int32),
                   det_cls=stack("det_cls", np.float64))
    return (stack("ranges", np.float32), _dev(cases[0]["tab"], np.float64), stack("cls", np.uint8)), nms


def _host(out):
    return {k: getattr(out, k).cpu().numpy() for k in OUT_FIELDS}


def dev_run(ops, cases):
    """The device's outputs for B cases (one N, one table, one set of settings) in one batch."""
    args, nms = _inputs(cases)
    return _host(ops.novel_segments(*args, **nms, **cases[0]["kw"]))


def check_case(ops, case, what):
    got, want = dev_run(ops, [case]), run_case(case)
    for k, dt in zip(OUT_FIELDS, OUT_DTYPES):
        assert got[k].dtype == dt and same_bits(got[k][0], want[k]), (what, k, got[k][0].tolist(), want[k].tolist())
    return want


# ------------------------------------------------------------------ 1. the device against the restatement
@pytest.mark.parametrize("name", sorted(rule_scenes()))
def test_rule_scenes(ops, name):
    check_case(ops, rule_scenes()[name], name)


FILL_PAIRS = ((1.0, 0.0), (0.5, 0.5), (-1.0, 0.25), (0.0, -1.0), (-0.5, -0.75), (0.25, 1.0), (0.0, 0.0))
FILL_RANGES = (0.5, 1.0, 2.5, np.inf, 0.9375)


def embedded(case, N, at):
    """The rule scene ``case`` with its n beams at beams at..at + n of a scan of N: around them beams of seven dyadic
    directions, five ranges and the five class bytes that are no member's."""
    n = len(case["ranges"])
    tab = np.asarray(case["tab"], np.float64)
    pairs = np.array([FILL_PAIRS[i % len(FILL_PAIRS)] for i in range(N)])
    ranges = np.array([FILL_RANGES[i % len(FILL_RANGES)] for i in range(N)], np.float32)
    cls = np.array([OTHER_BYTES[i % len(OTHER_BYTES)] for i in range(N)], np.uint8)
    pairs[at:at + n], ranges[at:at + n], cls[at:at + n] = tab[n:].reshape(n, 2), case["ranges"], case["cls"]
    big = dict(case, tab=np.concatenate([np.zeros(N), pairs.reshape(-1)]), ranges=ranges, cls=cls)
    if "inst" in case:
        inst, det_cls = np.zeros(N, np.int32), np.zeros(N)
        inst[at:at + n], det_cls[:n] = case["inst"], case["det_cls"]
        big.update(inst=inst, det_cls=det_cls)
    return big


@pytest.mark.parametrize("N", [512, 513, 4096])
def test_rule_scenes_embedded_in_long_scans(ops, N):
    scenes, beams = rule_scenes(), 0
    for name, case in scenes.items():
        if name.startswith("num_det"):
            continue                                           # num_det is clamped to the scan's own N: another scene
        n, small = len(case["ranges"]), run_case(case)
        nd = int(small["num_det"])
        for at in (0, (N - n) // 2 + 1, N - n):
            want = check_case(ops, embedded(case, N, at), (name, N, at))
            # the scene's own values, wherever it stands: the beams move by ``at``, nothing else does
            assert same_bits(want["instance_mask"][at:at + n], small["instance_mask"]) and \
                int(want["instance_mask"].sum()) == int(small["instance_mask"].sum())
            assert same_bits(want["det_first"][:nd], small["det_first"][:nd] + np.int32(at)) and \
                same_bits(want["det_last"][:nd], small["det_last"][:nd] + np.int32(at))
            for k in ("num_det", "seg_count"):
                assert same_bits(want[k], small[k]), (name, N, at, k)
            for k in ("det_xy", "det_cls", "det_count", "det_width2", "det_known"):
                assert same_bits(want[k][:n], small[k]) and not want[k][n:].any(), (name, N, at, k)
            beams += N
    print("N = %d: %d scenes at three placements, %d beams, every field the restatement's bits" % (N, len(scenes) - 2, beams))


@pytest.mark.parametrize("name", ["N 64", "N 65", "N 512", "N 512 dense", "N 513", "N 4096", "N 4096 dense"])
def test_pattern_cases(ops, name):
    want = check_case(ops, pattern_cases()[name], name)
    print("%s: %s segments (all, few, wide), %d rows, every field the restatement's bits"
          % (name, want["seg_count"].tolist(), int(want["num_det"])))
    assert int(want["num_det"]) > 0


def _cast_inputs(case, steps, origins):
    from planar_optical_flow_amd import ops
    stack = lambda k, dt: _dev(np.stack([np.asarray(s[k]) for s in steps]), dt)
    nms = {}
    if "inst" in steps[0]:
        nms = dict(instance_mask=stack("inst", np.int32), num_det=stack("num_det", np.int32),
                   det_cls=stack("det_cls", np.float64))
    state = ops.GridMapState(stack("grid", np.int16), _dev(np.stack(origins), np.float64))
    return (stack("ranges", np.float32), _dev(case["tab"], np.float64), stack("rot", np.float32),
            stack("trans", np.float64), state), nms


@pytest.mark.parametrize("name", ["rooms", "one tile", "128 x 192", "N 512", "N 513", "N 4096", "no NMS", "2048 x 2048",
                                  "N 1", "N 2", "N 3", "outside", "no rotation"])
def test_room_cases_cast_by_the_device(ops, name):
    from test_novel_segments import ROOM_REACH
    case = cast_device_cases()[name]
    sensors, reached = case["sensors"], np.zeros(2, np.int64)
    for steps in zip(*[s["steps"] for s in sensors]):
        args, nms = _cast_inputs(case, steps, [s["origin"] for s in sensors])
        cast = ops.grid_cast(*args, res=case["res"], **nms, **case["kw"])
        got = _host(ops.novel_segments(args[0], args[1], cast.point_class, **nms))
        classes = cast.point_class.cpu().numpy()
        for b, s in enumerate(steps):
            want = novel_segments_oracle(s["ranges"], case["tab"], classes[b], s.get("inst"), s.get("num_det"),
                                         s.get("det_cls"))
            for k in OUT_FIELDS:
                assert same_bits(got[k][b], want[k]), (name, b, k)
            reached += (want["seg_count"][0], want["num_det"])
    assert reached.tolist() == ROOM_REACH[name]                # what the restated cast reaches, the device's cast too


# ------------------------------------------------------------------ 2. determinism
def test_same_bits_at_five_batch_positions_and_in_two_runs(ops):
    cases = pattern_cases()
    me = cases["N 513"]
    other = dict(me, cls=np.roll(me["cls"], 7), ranges=np.roll(me["ranges"], 3))
    want, runs = run_case(me), []
    for pos in list(range(5)) + [2]:
        batch = [other] * 5
        batch[pos] = me
        got = dev_run(ops, batch)
        for k in OUT_FIELDS:
            assert same_bits(got[k][pos], want[k]), (pos, k)
        runs.append(got)
    for k in OUT_FIELDS:                                       # the two runs at position 2: every sensor's bits
        assert same_bits(runs[2][k], runs[5][k]), k
    assert not same_bits(runs[2]["instance_mask"][0], runs[2]["instance_mask"][2])


def test_two_replays_of_a_captured_launch_over_six_scans(ops):
    base = pattern_cases()["N 512"]
    B, N = 3, 512
    scans = [[dict(base, cls=np.roll(base["cls"], 5 * t + 11 * b), ranges=np.roll(base["ranges"], t + 2 * b),
                   inst=np.roll(base["inst"], 3 * t)) for b in range(B)] for t in range(6)]
    steps = [_inputs(batch) for batch in scans]
    args = [t.clone() if i == 1 else torch.zeros_like(t) for i, t in enumerate(steps[0][0])]
    nms = {k: torch.zeros_like(t) for k, t in steps[0][1].items()}
    out = ops.novel_segments_buffers(B, N)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                              # warm-up into buffers of its own
        ops.novel_segments(*args, **nms, **base["kw"])
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.novel_segments(*args, out=out, **nms, **base["kw"])
    rows = set()
    for _ in range(2):
        for t in range(6):
            for dst, src in zip(args, steps[t][0]):
                dst.copy_(src)
            for k in nms:
                nms[k].copy_(steps[t][1][k])
            graph.replay()
            got = _host(out)
            for b in range(B):
                want = run_case(scans[t][b])
                for k in OUT_FIELDS:
                    assert same_bits(got[k][b], want[k]), (t, b, k)
                rows.add(int(want["num_det"]))
    assert len(rows) > 1                                       # a replay with fewer rows zero-fills what the last one left


# ------------------------------------------------------------------ 3. refused calls
def test_refused_calls_leave_the_outputs_untouched(ops):
    from planar_optical_flow_amd import _lib
    from planar_optical_flow_amd._lib import POF_E_BADARG, POF_E_SHAPE, PofError
    rng = np.random.default_rng(1)
    base = pattern_cases()["N 64"]
    refusals = ((4097, {}, POF_E_SHAPE), (64, dict(jump=0.0), POF_E_BADARG), (64, dict(jump=float("nan")), POF_E_BADARG),
                (64, dict(max_width=-0.5), POF_E_BADARG), (64, dict(min_points=0), POF_E_BADARG),
                (64, dict(max_skip=-1), POF_E_BADARG), (64, dict(max_skip=65), POF_E_BADARG))
    for N, kw, code in refusals:
        case = base if N == 64 else dict(tab=np.zeros(3 * N), ranges=np.ones(N, np.float32), cls=np.full(N, 2, np.uint8))
        args, nms = _inputs([case])
        out = ops.novel_segments_buffers(1, N)
        for t in out:                                          # sentinels
            t.copy_(torch.from_numpy(rng.integers(1, 100, tuple(t.shape))).to(t.dtype))
        before = [t.cpu().numpy() for t in out]
        with pytest.raises(PofError if code == POF_E_SHAPE else AssertionError) as e:   # a bad argument is an assertion
            ops.novel_segments(*args, out=out, **nms, **dict(DEFAULTS, **kw))
        torch.cuda.synchronize()
        assert code == POF_E_BADARG or e.value.code == code, (N, kw)
        assert all(np.array_equal(a, t.cpu().numpy()) for a, t in zip(before, out)), (N, kw)
    # the NMS results in part: refused by the wrapper and by the entry point itself
    args, nms = _inputs([base])
    out = ops.novel_segments_buffers(1, 64)
    for part in (("instance_mask",), ("num_det", "det_cls"), ("instance_mask", "det_cls")):
        with pytest.raises(ValueError):
            ops.novel_segments(*args, out=out, **{k: nms[k] for k in part})
    ptr = lambda t: t.data_ptr()
    rc = _lib.load().pof_novel_segments(ptr(args[0]), ptr(args[1]), ptr(args[2]), ptr(nms["instance_mask"]), None,
                                        ptr(nms["det_cls"]), 0.5, 0.3, 2, 3, 1.0, 1, 64, *[ptr(t) for t in out], None)
    torch.cuda.synchronize()
    assert rc == POF_E_BADARG and not any(t.any() for t in out)
    with pytest.raises(ValueError):
        ops.novel_segments(args[0], args[1], args[2][:, :63].contiguous())              # classes of another scan
    with pytest.raises(ValueError):
        ops.novel_segments(*args, out=ops.novel_segments_buffers(1, 65))
    with pytest.raises(ValueError):
        ops.novel_segments(*args, out=ops.novel_segments_buffers(2, 64))
    with pytest.raises(TypeError):
        ops.novel_segments(args[0], args[1], args[2].to(torch.int32))
    empty = ops.novel_segments(args[0][:0], args[1], args[2][:0])
    assert empty.instance_mask.shape == (0, 64) and empty.num_det.shape == (0,) and empty.seg_count.shape == (0, 3)
    # the next good call works, with ``out=`` and without it
    o = ops.novel_segments(*args, out=out, **nms, **base["kw"])
    fresh = ops.novel_segments(*args, **nms, **base["kw"])
    want = run_case(base)
    assert o is out and type(fresh) is ops.NovelSegments
    for k, a, b in zip(OUT_FIELDS, o, fresh):
        assert a.data_ptr() != b.data_ptr() and same_bits(a[0].cpu().numpy(), want[k]) and \
            same_bits(b[0].cpu().numpy(), want[k]), k


# ------------------------------------------------------------------ 4. the reference-shaped class
SEG_KEYS = (("seg_xy", "det_xy"), ("seg_cls", "det_cls"), ("seg_points", "det_count"), ("seg_first", "det_first"),
            ("seg_last", "det_last"), ("seg_width2", "det_width2"), ("seg_known", "det_known"))


def test_occupancy_grid_novel_segments_is_the_restated_cast_then_segments(ops):
    import src.utils.utils as u
    scene = people_scene(24, 8, 0.25)
    N, res, size = 450, 0.1, (128, 192)
    phi = scene["tab"][:N]
    rng = np.random.default_rng(3)
    og = u.OccupancyGrid(phi, res=res, size=size, max_range=10.0, min_dist=0.5, cls_thresh=0.4)
    tab = u._table_for(phi)
    htab = tab.cpu().numpy()
    grid = np.zeros(size, np.int16)
    origin = scene["poses"][0][:2] - 0.5 * res * np.array([192.0, 128.0])
    cls, reg = rng.uniform(0.05, 0.95, (N, 1)), rng.normal(0.0, 0.05, (N, 2))
    kept = 0
    for t, s in enumerate(scene["scans"]):
        gated = t % 3 != 1                                     # some scans without predictions
        preds = (cls, reg) if gated else ()
        got = og.novel_segments(s["ranges"], scene["poses"][t], *preds, tol=0.15, jump=0.25, min_points=2)
        upd = og.update(s["ranges"], scene["poses"][t], *preds)    # behind it, as with ``cast``
        nms = ()
        if gated:
            ranges = _dev(s["ranges"], np.float32).reshape(1, N)
            _, dc, num, inst = ops.nms_predicted_center(ranges, tab, _dev(cls[:, 0], np.float64).reshape(1, N),
                                                        _dev(reg, np.float64).reshape(1, N, 2), 0.5)
            nms = tuple(v[0].cpu().numpy() for v in (inst, num, dc))
        rot, trans, _ = u._pose_terms(scene["poses"][t][None])
        cast = grid_cast_oracle(s["ranges"], htab, rot[0], trans[0], grid, origin, res, *nms, max_range=10.0, tol=0.15)
        want = novel_segments_oracle(s["ranges"], htab, cast["point_class"], *nms, cls_thresh=0.4, jump=0.25,
                                     min_points=2)
        m = int(want["num_det"])
        kept += m
        assert same_bits(got["point_class"], cast["point_class"]) and same_bits(got["exp_range"], cast["exp_range"])
        assert got["seg_num"] == m and same_bits(got["seg_instance_mask"], want["instance_mask"]) and \
            same_bits(got["seg_count"], want["seg_count"]), t
        for name, k in SEG_KEYS:
            assert same_bits(got[name], want[k][:m]), (t, name)
        assert ("instance_mask" in got) == gated               # the NMS's own mask keeps its name
        grid_map_oracle(s["ranges"], htab, rot[0], trans[0], grid, origin, res, *nms, cls_thresh=0.4, max_range=10.0)
        assert np.array_equal(og.logodds, grid) and np.array_equal(og.origin, origin), t
        assert upd["point_prior"].shape == (N,)
    assert kept > 0
    for bad in (dict(max_range=5.0), dict(cls_thresh=0.5), dict(jumps=1.0)):
        with pytest.raises(ValueError, match="unknown novel_segments settings"):
            og.novel_segments(scene["scans"][0]["ranges"], scene["poses"][0], **bad)
    fresh = u.OccupancyGrid(phi, res=res, size=64)
    first = fresh.novel_segments(scene["scans"][0]["ranges"], (1.0, 2.0, 0.5))         # centres the grid as update would
    assert fresh.origin.tolist() == [1.0 - 3.2, 2.0 - 3.2] and first["seg_num"] == 0 and first["seg_xy"].shape == (0, 2)


# ------------------------------------------------------------------ 5. the layout claim
def test_the_record_feeds_person_motion_and_track_update(ops):
    """``ops.person_motion(ranges, tab, *rec[:4], rot, trans, state)`` and ``ops.track_update`` on its result over a
    12-scan ``people_scene`` whose map is gated by the scene's detections equal the restated chain --
    ``person_motion_oracle`` and ``track_step`` on the restatement's record -- bit for bit (in person_motion's outputs a
    NaN equals a NaN: a row without a partner; the track state has none)."""
    scene = people_scene(1, 12, 0.25)
    N, M, res, size = 450, 16, 0.1, 256
    origin = scene["poses"][0, :2] - 0.5 * res * size
    grid = np.zeros((size, size), np.int16)
    tab = _dev(scene["tab"], np.float64)
    pm_state, tracks = ops.person_motion_state(1, N), ops.track_buffers(1, M, N)
    want_pm, want_tr = motion_state(N), new_track_state(M, N)
    rows = pairs = 0
    for t, s in enumerate(scene["scans"]):
        cast = grid_cast_oracle(s["ranges"], scene["tab"], s["rot"], s["trans"], grid, origin, res)
        grid_map_oracle(s["ranges"], scene["tab"], s["rot"], s["trans"], grid, origin, res, s["inst"], s["num_det"],
                        s["det_cls"])
        ranges = _dev(s["ranges"], np.float32).reshape(1, N)
        rec = ops.novel_segments(ranges, tab, _dev(cast["point_class"], np.uint8).reshape(1, N))
        want = novel_segments_oracle(s["ranges"], scene["tab"], cast["point_class"])
        for k, v in zip(OUT_FIELDS, rec):
            assert same_bits(v[0].cpu().numpy(), want[k]), (t, k)
        rot, trans = _dev(s["rot"], np.float32).reshape(1, 2, 2), _dev(s["trans"], np.float64).reshape(1, 2)
        pm = ops.person_motion(ranges, tab, *rec[:4], rot, trans, pm_state)
        ops.track_update(pm.det_xy_world, pm.det_flow, pm.det_valid, rec.num_det, rec.instance_mask, tracks)
        o = person_motion_oracle(s["ranges"], scene["tab"], want["instance_mask"], want["num_det"], want["det_xy"],
                                 want["det_cls"], s["rot"], s["trans"], want_pm)
        for k, v in o.items():
            assert same_bits_nan(getattr(pm, k)[0].cpu().numpy(), np.asarray(v, getattr(pm, k).cpu().numpy().dtype)), (t, k)
        track_step(want_tr, o["det_xy_world"], o["det_flow"], o["det_valid"], want["num_det"], want["instance_mask"])
        for k in TRACK_INT:
            assert np.array_equal(getattr(tracks, k)[0].cpu().numpy(), want_tr[k]), (t, k)
        for k in TRACK_FLOAT:
            got = getattr(tracks, k)[0].cpu().numpy()
            assert same_bits(got, want_tr[k]), (t, k, float(np.abs(got - want_tr[k]).max(initial=0.0)))
        rows, pairs = rows + int(want["num_det"]), pairs + int((o["det_prev"] >= 0).sum())
    print("12 scans: %d segment rows, %d paired with the scan before, %d tracks born" % (rows, pairs, int(want_tr["next_id"]) - 1))
    assert rows > 10 and pairs > 5 and int(want_tr["next_id"]) > 1 and bool((want_tr["track_confirmed"] != 0).any())


# ------------------------------------------------------------------ 6. streaming detector
STREAM_SIZE, STREAM_RES, STREAM_RANGE = 192, 0.05, 6.0


def _stream_model(seed):
    from planar_optical_flow_amd.src.depracted.model.dr_spaam import SpatialDROW
    torch.manual_seed(seed)
    return SpatialDROW(num_scans=5, num_pts=56, alpha=0.5, window_size=11, pedestrian_only=True).cuda().eval()


def drives_with_a_walker():
    """tests/test_grid_scroll_gpu.two_drives with somebody crossing each sensor's view: in scan t a run of 14 beams,
    25 beams further along than in the scan before, ends 1.2 m in front of the sensor -- in space the scans before saw
    empty, so from the third scan on the cast calls those points NOVEL."""
    from test_grid_scroll_gpu import two_drives
    scans, poses = two_drives()
    scans = scans.copy()
    for t in range(len(scans)):
        for b in range(2):
            at = 40 + 25 * t + 60 * b
            scans[t, b, at:at + 14] = np.float32(1.2) + np.float32(0.01) * np.arange(14, dtype=np.float32)
    return scans, poses


def _snapshot(det):
    """Everything the cast, the segments, the scroll and the grid stage read and leave behind, on the host."""
    state, _ = det.grid_map()
    snap = {"rot": det._pose_rot, "trans": det._pose_trans, "grid": state.grid, "origin": state.origin,
            "point_class": det.grid_cast().point_class, "shift": det._gs_out.shift, "offset": det._gs_state.offset}
    if det._dets is not None:
        _, conf, num, inst = det._dets
        snap.update(nms_cls=conf, nms_num=num, nms_inst=inst)
    if det._ns_kw is not None:
        snap.update(zip(OUT_FIELDS, det.novel_segments()))
    return {k: v.detach().cpu().numpy().copy() for k, v in snap.items()}


def _restated_step(scan, tab, g, b, grid, origin, base, offset, gate, seg_kw):
    """One sensor's scroll -> cast -> segments -> map on the step's own pose and NMS records; the grid is advanced in
    place.  ``gate``: "nms" or "segments".  -> (the restated segments, the restated cast)."""
    grid_scroll_oracle(g["trans"][b], grid, origin, base, offset, STREAM_RES, 64)
    nms = (g["nms_inst"][b], g["nms_num"][b], g["nms_cls"][b]) if "nms_inst" in g else (None, None, None)
    cast = grid_cast_oracle(scan, tab, g["rot"][b], g["trans"][b], grid, origin, STREAM_RES, *nms,
                            **dict(CAST_DEFAULTS, max_range=STREAM_RANGE))
    seg = novel_segments_oracle(scan, tab, cast["point_class"], *nms, **seg_kw)
    by = (seg["instance_mask"], seg["num_det"], seg["det_cls"]) if gate == "segments" else nms
    grid_map_oracle(scan, tab, g["rot"][b], g["trans"][b], grid, origin, STREAM_RES, *by,
                    **dict(MAP_DEFAULTS, max_range=STREAM_RANGE))
    return seg, cast


@pytest.mark.parametrize("ego", ["keyframe", "scan_match"])
@pytest.mark.parametrize("gate_map", [False, True])
def test_streaming_detector_eager_graph_and_restated_chain(ego, gate_map):
    from planar_optical_flow_amd.streaming import StreamingDetector
    B, size, res, T = 2, STREAM_SIZE, STREAM_RES, 12
    scans, poses = drives_with_a_walker()
    model = _stream_model(13)
    seg_set = dict(jump=0.25, min_points=4)
    kw = dict(batch=B, cls_thresh=0.5, grid_map=dict(size=size, res=res, max_range=STREAM_RANGE),
              ego_motion=dict(method=ego), grid_scroll=dict(margin=64), grid_cast=dict(max_range=STREAM_RANGE))
    if not gate_map:
        kw["nms_min_dist"] = 0.5                               # the NMS's results reach det_known
    eager = StreamingDetector(model, graph=False, novel_segments=dict(seg_set, gate_map=gate_map), **kw)
    graphed = StreamingDetector(model, graph=True, novel_segments=dict(seg_set, gate_map=gate_map), **kw)
    parent = StreamingDetector(model, graph=True, **kw)         # what the detector is without the stage
    assert parent._ns_kw is None and not hasattr(parent, "_ns_out") and len(eager._stages) == len(parent._stages) + 1
    names = [s.launch.__name__ for s in graphed._stages]
    at = names.index("_novel_segments_stage")
    assert names[at - 1] == "_grid_cast_stage" and names[at + 1] == "_grid_stage"
    assert graphed._ns_kw == dict(DEFAULTS, **seg_set) and graphed._ns_gates is gate_map
    tab = graphed.tab.cpu().numpy()
    seg_kw = dict(DEFAULTS, **seg_set)
    half = 0.5 * res * size
    start = poses[0][:, :2]

    def run():
        grids = [np.zeros((size, size), np.int16) for _ in range(B)]
        origins, offsets = [start[b] - half for b in range(B)], [np.zeros(2, np.int32) for _ in range(B)]
        kept = known = differs = 0
        for det in (eager, graphed, parent):
            det.reset(pose=poses[0])
        for t in range(T):
            for det in (eager, graphed, parent):
                if t == 0 and det is not parent:
                    with pytest.raises(RuntimeError, match="novel_segments"):
                        det.novel_segments()
                det(torch.from_numpy(scans[t]).cuda())
            e, g = _snapshot(eager), _snapshot(graphed)
            for k in e:
                assert same_bits(e[k], g[k]), (t, k)           # eager and replayed: identical bits
            for b in range(B):
                want, _ = _restated_step(scans[t, b], tab, g, b, grids[b], origins[b], start[b] - half, offsets[b],
                                         "segments" if gate_map else "nms", seg_kw)
                assert g["origin"][b].tobytes() == origins[b].tobytes(), (t, b)
                for k in OUT_FIELDS:
                    assert same_bits(g[k][b], want[k]), (t, b, k)
                assert np.array_equal(g["grid"][b], grids[b]), (t, b)
                kept, known = kept + int(want["num_det"]), known + int(want["det_known"].sum())
            same = torch.equal(parent._gm_state.grid, graphed._gm_state.grid)
            if not gate_map:                                   # the stage writes nothing of the others: the parent's grid
                assert same and torch.equal(parent._gm_out.point_prior, graphed._gm_out.point_prior)
            differs += not same
        assert graphed.novel_segments() is graphed._ns_out and type(graphed._ns_out).__name__ == "NovelSegments"
        return kept, known, differs

    kept, known, differs = run()
    print("ego=%s gate_map=%s: %d segments kept over %d scans of %d sensors, %d of their points known to the NMS, the "
          "grid differs from the ungated one after %d scans" % (ego, gate_map, kept, T, B, known, differs))
    assert kept > 0                                            # the scene keeps a segment ...
    assert (differs > 0) == gate_map                           # ... and gated by it the map is another one
    assert graphed._graph is not None and eager._graph is None
    for det in (eager, graphed):
        det.reset(pose=(1.0, -2.0, 0.25))
        with pytest.raises(RuntimeError):
            det.novel_segments()
    assert run() == (kept, known, differs)                     # the same sequence again behind a reset


def test_streaming_detector_constructor_rules():
    from planar_optical_flow_amd.streaming import StreamingDetector
    model = _stream_model(13)
    grid = dict(grid_map=dict(size=64))
    with pytest.raises(ValueError, match="grid_cast"):
        StreamingDetector(model, novel_segments=dict(), **grid)
    with pytest.raises(ValueError, match="grid_cast"):
        StreamingDetector(model, novel_segments=dict())
    with pytest.raises(ValueError, match="gate_map with nms_min_dist is not built"):
        StreamingDetector(model, nms_min_dist=0.5, grid_cast=dict(), novel_segments=dict(gate_map=True), **grid)
    for bad in (dict(jump=0.0), dict(max_width=-0.1), dict(min_points=0), dict(max_skip=65), dict(max_skip=-1)):
        with pytest.raises(ValueError, match="novel_segments"):
            StreamingDetector(model, grid_cast=dict(), novel_segments=bad, **grid)
    for bad in (dict(cls_thresh=0.5), dict(res=0.1), dict(jumps=1.0)):
        with pytest.raises(ValueError, match="unknown novel_segments settings"):
            StreamingDetector(model, grid_cast=dict(), novel_segments=bad, **grid)
    plain = StreamingDetector(model, grid_cast=dict(), **grid)
    assert plain._ns_kw is None and not any(name.startswith("_ns_") and name != "_ns_kw" for name in dir(plain))
    with pytest.raises(RuntimeError, match="novel_segments"):
        plain.novel_segments()
    # a pose per call, with the NMS and without the gate: allowed, and the first scan of a sequence runs the stage
    det = StreamingDetector(model, nms_min_dist=0.5, cls_thresh=0.3, grid_cast=dict(), novel_segments=dict(max_skip=0),
                            **grid)
    assert det._ns_kw == dict(cls_thresh=0.3, jump=0.3, max_skip=0, min_points=3, max_width=1.0) and not det._ns_gates
    det(torch.zeros(450).cuda() + 3.0, pose=(1.0, 2.0, 0.5))
    o = det.novel_segments()
    assert o is det._ns_out and not bool(o.num_det.any()) and o.seg_count.tolist() == [[0, 0, 0]]   # an empty map: no NOVEL
