"""Merged detections (pof_merge_detections, N18) on the GPU: the device against the NumPy restatement of
tests/test_merge_detections.py, every one of the eleven outputs BIT FOR BIT (the stage is integers and bitwise copies:
there is no tolerance) -- on the rule scenes at their own size and embedded at the start, the middle and the end of scans
of 512, 513 and 4096 points (one wave up to 512 points, 512 threads beyond), on the seeded patterns; at five batch
positions, in two runs and in two replays of a captured launch; refused calls; through
``utils.OccupancyGrid.merged_detections``; the record as the input of ``ops.person_motion`` and ``ops.track_update``; and
as a stage of the streaming detector, eager and replayed, against the restated chain scroll -> cast -> segments -> merge
-> person motion -> tracks -> map -> track map, with and without the NMS and with and without the merged gate."""
import os
import sys

import numpy as np
import pytest
import torch

from test_grid_cast import DEFAULTS as CAST_DEFAULTS, grid_cast_oracle
from test_grid_map import DEFAULTS as MAP_DEFAULTS, OUT_FIELDS as MAP_FIELDS, grid_map_oracle
from test_grid_scroll import grid_scroll_oracle
from test_merge_detections import (DEFAULTS, OUT_DTYPES, OUT_FIELDS, lowered_scene, merge_detections_oracle,
                                   pattern_cases, rule_scenes, run_case)
from test_novel_segments import DEFAULTS as SEG_DEFAULTS, OUT_FIELDS as SEG_FIELDS, novel_segments_oracle, same_bits
from test_person_motion import motion_state, people_scene, person_motion_oracle, same_bits as same_bits_nan
from test_track_map import (DEFAULTS as TM_DEFAULTS, OUT_FIELDS as TM_FIELDS, STATE_FIELDS as TM_STATE,
                            new_state as new_tm_state, track_map_oracle)
from test_tracks import FLOAT_FIELDS as TRACK_FLOAT, INT_FIELDS as TRACK_INT, new_state as new_track_state, track_step

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "planar_optical_flow_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

REC_DTYPES = (np.int32, np.int32, np.float64, np.float64)


@pytest.fixture(scope="module")
def ops():
    from planar_optical_flow_amd import ops as _ops
    return _ops


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def _inputs(cases):
    """B cases of one N as device tensors: the four of B, and A's keywords ({} without A)."""
    stack = lambda rec, i: _dev(np.stack([np.asarray(c[rec][i]) for c in cases]), REC_DTYPES[i])
    b = tuple(stack("b", i) for i in range(4))
    a = {}
    if cases[0]["a"] is not None:
        a = dict(zip(("instance_mask", "num_det", "det_xy", "det_cls"), (stack("a", i) for i in range(4))))
    return b, a


def _host(out):
    return {k: getattr(out, k).cpu().numpy() for k in OUT_FIELDS}


def dev_run(ops, cases):
    """The device's outputs for B cases (one N, one set of settings) in one batch."""
    b, a = _inputs(cases)
    return _host(ops.merge_detections(*b, **a, **cases[0]["kw"]))


def check_case(ops, case, what):
    got, want = dev_run(ops, [case]), run_case(case)
    for k, dt in zip(OUT_FIELDS, OUT_DTYPES):
        assert got[k].dtype == dt and same_bits(got[k][0], want[k]), (what, k, got[k][0].tolist(), want[k].tolist())
    return want


# ------------------------------------------------------------------ 1. the device against the restatement
@pytest.mark.parametrize("name", sorted(rule_scenes()))
def test_rule_scenes(ops, name):
    check_case(ops, rule_scenes()[name], name)


FILL_IDS = (0, -1, 9, 0, 2 ** 31 - 1, -2 ** 31, 4097)           # nobody's in a scene of at most 8 rows


def embedded(case, N, at):
    """The rule scene ``case`` with its n points at the points at..at + n of a scan of N: around them ids that are
    nobody's, behind its rows centres and scores that nothing may read."""
    def grown(rec):
        inst, num, xy, cls = rec
        n = len(inst)
        big_inst = np.array([FILL_IDS[i % len(FILL_IDS)] for i in range(N)], np.int32)
        big_inst[at:at + n] = inst
        big_xy, big_cls = np.full((N, 2), 7.0), np.full(N, 0.875)
        big_xy[:n], big_cls[:n] = xy, cls
        return big_inst, num, big_xy, big_cls
    return dict(case, b=grown(case["b"]), a=None if case["a"] is None else grown(case["a"]))


@pytest.mark.parametrize("N", [512, 513, 4096])
def test_rule_scenes_embedded_in_long_scans(ops, N):
    scenes, points = rule_scenes(), 0
    for name, case in scenes.items():
        n, small = len(case["b"][0]), run_case(case)
        # a count beyond N, or rows up to N, mean another thing in a longer scan: the device still equals the restatement
        moves = not name.startswith(("num_det", "nA N"))
        for at in (0, (N - n) // 2 + 1, N - n):
            want = check_case(ops, embedded(case, N, at), (name, N, at))
            points += N
            if not moves:
                continue
            # the scene's own values, wherever it stands: the points move by ``at``, nothing else does
            assert same_bits(want["instance_mask"][at:at + n], small["instance_mask"]) and \
                int((want["instance_mask"] != 0).sum()) == int((small["instance_mask"] != 0).sum()), (name, N, at)
            for k in ("num_det", "merge_count"):
                assert same_bits(want[k], small[k]), (name, N, at, k)
            for k in OUT_FIELDS[2:10]:
                assert same_bits(want[k][:n], small[k]) and (want[k][n:] == (-1 if k == "b_row" else 0)).all(), \
                    (name, N, at, k)
    print("N = %d: %d scenes at three placements, %d points, every field the restatement's bits" % (N, len(scenes), points))


@pytest.mark.parametrize("name", sorted(pattern_cases()))
def test_pattern_cases(ops, name):
    want = check_case(ops, pattern_cases()[name], name)
    print("%s: merge_count %s, every field the restatement's bits" % (name, want["merge_count"].tolist()))
    assert int(want["merge_count"][1]) > 0 and int(want["merge_count"][2]) > 0


# ------------------------------------------------------------------ 2. determinism
def _rolled(case, by):
    """Another case of the same size: both masks rolled along the scan."""
    (bi, bn, bx, bc), (ai, an, ax, ac) = case["b"], case["a"]
    return dict(case, b=(np.roll(bi, by), bn, bx, bc), a=(np.roll(ai, 2 * by + 1), an, ax, ac))


def test_same_bits_at_five_batch_positions_and_in_two_runs(ops):
    me = pattern_cases()["N 513"]
    other = _rolled(me, 7)
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


def test_two_replays_of_a_captured_launch_over_six_inputs(ops):
    base = pattern_cases()["N 512"]
    B, N = 3, 512
    steps = [[_rolled(base, 5 * t + 11 * b) for b in range(B)] for t in range(6)]
    for t in (2, 5):                                           # fewer rows than the step before: the zero-fill
        steps[t] = [dict(c, b=(c["b"][0], np.int32(9 + b), c["b"][2], c["b"][3]),
                         a=(c["a"][0], np.int32(3), c["a"][2], c["a"][3])) for b, c in enumerate(steps[t])]
    tensors = [_inputs(batch) for batch in steps]
    b_in = [torch.zeros_like(t) for t in tensors[0][0]]
    a_in = {k: torch.zeros_like(t) for k, t in tensors[0][1].items()}
    out = ops.merge_detections_buffers(B, N)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                              # warm-up into buffers of its own
        ops.merge_detections(*b_in, **a_in, **base["kw"])
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.merge_detections(*b_in, out=out, **a_in, **base["kw"])
    rows = set()
    for _ in range(2):
        for t in range(6):
            for dst, src in zip(b_in, tensors[t][0]):
                dst.copy_(src)
            for k in a_in:
                a_in[k].copy_(tensors[t][1][k])
            graph.replay()
            got = _host(out)
            for b in range(B):
                want = run_case(steps[t][b])
                for k in OUT_FIELDS:
                    assert same_bits(got[k][b], want[k]), (t, b, k)
                rows.add(int(want["num_det"]))
    assert len(rows) > 2 and min(rows) < 20 < max(rows)


# ------------------------------------------------------------------ 3. refused calls
def test_refused_calls_leave_the_outputs_untouched(ops):
    from planar_optical_flow_amd import _lib
    from planar_optical_flow_amd._lib import POF_E_BADARG, POF_E_SHAPE, PofError
    rng = np.random.default_rng(1)
    base = pattern_cases()["N 64"]

    def sentinels(N):
        out = ops.merge_detections_buffers(1, N)
        for t in out:
            t.copy_(torch.from_numpy(rng.integers(1, 100, tuple(t.shape))).to(t.dtype))
        return out, [t.cpu().numpy() for t in out]

    for N, kw, code in ((4097, {}, POF_E_SHAPE), (64, dict(absorb_pct=-1), POF_E_BADARG),
                        (64, dict(absorb_pct=102), POF_E_BADARG)):
        case = base if N == 64 else dict(b=(np.ones(N, np.int32), np.int32(1), np.zeros((N, 2)), np.ones(N)), a=None)
        b, a = _inputs([case])
        out, before = sentinels(N)
        with pytest.raises(PofError if code == POF_E_SHAPE else AssertionError) as e:   # a bad argument is an assertion
            ops.merge_detections(*b, out=out, **a, **dict(DEFAULTS, **kw))
        torch.cuda.synchronize()
        assert code == POF_E_BADARG or e.value.code == code, (N, kw)
        assert all(np.array_equal(x, t.cpu().numpy()) for x, t in zip(before, out)), (N, kw)
    # the primary record in part: refused by the wrapper and by the entry point itself
    b, a = _inputs([base])
    out, before = sentinels(64)
    names = list(a)
    for part in [names[:j] + names[j + 1:] for j in range(4)] + [[k] for k in names]:
        with pytest.raises(ValueError, match="come together or not at all"):
            ops.merge_detections(*b, out=out, **{k: a[k] for k in part})
    ptr = lambda t: None if t is None else t.data_ptr()
    for j in range(4):
        prim = [None if i == j else a[k] for i, k in enumerate(names)]
        rc = _lib.load().pof_merge_detections(*[ptr(t) for t in b], *[ptr(t) for t in prim], 0.5, 50, 1, 64,
                                              *[ptr(t) for t in out], None)
        assert rc == POF_E_BADARG, j
    torch.cuda.synchronize()
    assert all(np.array_equal(x, t.cpu().numpy()) for x, t in zip(before, out))
    with pytest.raises(ValueError):
        ops.merge_detections(b[0], b[1], b[2][:, :63].contiguous(), b[3])               # centres of another scan
    with pytest.raises(ValueError):
        ops.merge_detections(*b, out=ops.merge_detections_buffers(1, 65))
    with pytest.raises(ValueError):
        ops.merge_detections(*b, out=ops.merge_detections_buffers(2, 64))
    with pytest.raises(TypeError):
        ops.merge_detections(b[0].to(torch.int64), *b[1:])
    empty = ops.merge_detections(*[t[:0] for t in b])
    assert empty.instance_mask.shape == (0, 64) and empty.num_det.shape == (0,) and empty.merge_count.shape == (0, 4)
    # the next good call works, with ``out=`` and without it
    o = ops.merge_detections(*b, out=out, **a, **base["kw"])
    fresh = ops.merge_detections(*b, **a, **base["kw"])
    want = run_case(base)
    assert o is out and type(fresh) is ops.MergedDetections
    for k, x, y in zip(OUT_FIELDS, o, fresh):
        assert x.data_ptr() != y.data_ptr() and same_bits(x[0].cpu().numpy(), want[k]) and \
            same_bits(y[0].cpu().numpy(), want[k]), k


# ------------------------------------------------------------------ 4. the reference-shaped class
MERGED_KEYS = (("merged_xy", "det_xy"), ("merged_cls", "det_cls"), ("merged_points", "det_points"),
               ("merged_src", "det_src"), ("merged_row", "det_row"))


def test_occupancy_grid_merged_detections_is_the_restated_chain(ops):
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
    rows = appended = 0
    for t, s in enumerate(scene["scans"]):
        gated = t % 3 != 1                                     # some scans without predictions
        preds = (cls, reg) if gated else ()
        got = og.merged_detections(s["ranges"], scene["poses"][t], *preds, tol=0.15, jump=0.25, min_points=2,
                                   absorb_pct=40)
        og.update(s["ranges"], scene["poses"][t], *preds)      # behind it, as with ``cast``
        nms, prim = (), ()
        if gated:
            ranges = _dev(s["ranges"], np.float32).reshape(1, N)
            xy, dc, num, inst = ops.nms_predicted_center(ranges, tab, _dev(cls[:, 0], np.float64).reshape(1, N),
                                                         _dev(reg, np.float64).reshape(1, N, 2), 0.5)
            nms = tuple(v[0].cpu().numpy() for v in (inst, num, dc))
            prim = (nms[0], nms[1], xy[0].cpu().numpy(), nms[2])
        rot, trans, _ = u._pose_terms(scene["poses"][t][None])
        cast = grid_cast_oracle(s["ranges"], htab, rot[0], trans[0], grid, origin, res, *nms, max_range=10.0, tol=0.15)
        seg = novel_segments_oracle(s["ranges"], htab, cast["point_class"], *nms, cls_thresh=0.4, jump=0.25,
                                    min_points=2)
        want = merge_detections_oracle(seg["instance_mask"], seg["num_det"], seg["det_xy"], seg["det_cls"], *prim,
                                       cls_thresh=0.4, absorb_pct=40)
        m, k_seg = int(want["num_det"]), int(seg["num_det"])
        rows, appended = rows + m, appended + int(want["merge_count"][1])
        assert got["seg_num"] == k_seg and same_bits(got["seg_instance_mask"], seg["instance_mask"]), t
        assert got["merged_num"] == m and same_bits(got["merged_instance_mask"], want["instance_mask"]) and \
            same_bits(got["merge_count"], want["merge_count"]) and same_bits(got["seg_row"], want["b_row"][:k_seg]), t
        for name, k in MERGED_KEYS:
            assert same_bits(got[name], want[k][:m]), (t, name)
        assert ("instance_mask" in got) == gated               # the NMS's own mask keeps its name
        grid_map_oracle(s["ranges"], htab, rot[0], trans[0], grid, origin, res, *nms, cls_thresh=0.4, max_range=10.0)
        assert np.array_equal(og.logodds, grid), t
    print("8 scans: %d merged rows, %d of them appended segments" % (rows, appended))
    assert rows > appended > 0
    for bad in (dict(max_range=5.0), dict(cls_thresh=0.5), dict(absorb=1)):
        with pytest.raises(ValueError, match="unknown"):
            og.merged_detections(scene["scans"][0]["ranges"], scene["poses"][0], **bad)


# ------------------------------------------------------------------ 5. the layout claim
def test_the_record_feeds_person_motion_and_track_update(ops):
    """``ops.person_motion(ranges, tab, *merged[:4], rot, trans, state)`` and ``ops.track_update`` on its result over a
    12-scan ``people_scene`` whose odd-numbered people have their scores lowered equal the restated chain --
    ``person_motion_oracle`` and ``track_step`` on the restatement's merged record -- bit for bit (in person_motion's
    outputs a NaN equals a NaN: a row without a partner; the track state has none)."""
    scene, low = lowered_scene(1, 12, 0.25)
    N, M, res, size = 450, 16, 0.1, 256
    origin = scene["poses"][0, :2] - 0.5 * res * size
    grid = np.zeros((size, size), np.int16)
    tab = _dev(scene["tab"], np.float64)
    pm_state, tracks = ops.person_motion_state(1, N), ops.track_buffers(1, M, N)
    want_pm, want_tr = motion_state(N), new_track_state(M, N)
    rows = appended = 0
    born = set()
    for t, s in enumerate(scene["scans"]):
        cast = grid_cast_oracle(s["ranges"], scene["tab"], s["rot"], s["trans"], grid, origin, res)
        ranges = _dev(s["ranges"], np.float32).reshape(1, N)
        a = dict(instance_mask=_dev(s["inst"], np.int32).reshape(1, N), num_det=_dev(s["num_det"], np.int32).reshape(1),
                 det_xy=_dev(s["det_xy"], np.float64).reshape(1, N, 2), det_cls=_dev(s["det_cls"], np.float64).reshape(1, N))
        seg = ops.novel_segments(ranges, tab, _dev(cast["point_class"], np.uint8).reshape(1, N),
                                 **{k: v for k, v in a.items() if k != "det_xy"})
        rec = ops.merge_detections(*seg[:4], **a)
        want_seg = novel_segments_oracle(s["ranges"], scene["tab"], cast["point_class"], s["inst"], s["num_det"],
                                         s["det_cls"])
        want = merge_detections_oracle(want_seg["instance_mask"], want_seg["num_det"], want_seg["det_xy"],
                                       want_seg["det_cls"], s["inst"], s["num_det"], s["det_xy"], s["det_cls"])
        for k, v in zip(OUT_FIELDS, rec):
            assert same_bits(v[0].cpu().numpy(), want[k]), (t, k)
        grid_map_oracle(s["ranges"], scene["tab"], s["rot"], s["trans"], grid, origin, res, want["instance_mask"],
                        want["num_det"], want["det_cls"])
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
            assert same_bits(getattr(tracks, k)[0].cpu().numpy(), want_tr[k]), (t, k)
        nA = int(want["merge_count"][0])
        rows, appended = rows + int(want["num_det"]), appended + int(want["merge_count"][1])
        live = want_tr["track_id"] != 0
        born |= set(want_tr["track_id"][live & (want_tr["track_det"] >= nA)].tolist())
    print("12 scans: %d merged rows, %d of them appended, %d tracks, %d of them held an appended row"
          % (rows, appended, int(want_tr["next_id"]) - 1, len(born)))
    assert appended > 0 and len(born) > 0 and int(want_tr["next_id"]) > 1


# ------------------------------------------------------------------ 6. streaming detector
STREAM_SIZE, STREAM_RES, STREAM_RANGE, STREAM_M = 192, 0.05, 6.0, 64
PERSON = dict(person_motion=dict(), tracks=dict(), track_map=dict())
CASES = {"keyframe": ("keyframe", True, True), "scan_match": ("scan_match", True, True),
         "keyframe, the NMS's gate": ("keyframe", True, False), "scan_match, no NMS": ("scan_match", False, True)}


def _snapshot(det):
    """Everything the stages of the table read and leave behind, on the host."""
    snap = {"rot": det._pose_rot, "trans": det._pose_trans, "grid": det._gm_state.grid, "origin": det._gm_state.origin,
            "point_class": det.grid_cast().point_class, "offset": det._gs_state.offset}
    snap.update({"gm_" + k: v for k, v in det._gm_out._asdict().items()})
    snap.update({"ns_" + k: v for k, v in det._ns_out._asdict().items()})
    if det._dets is not None:
        xy, conf, num, inst = det._dets
        snap.update(nms_xy=xy, nms_cls=conf, nms_num=num, nms_inst=inst)
    if det._mg_kw is not None:
        snap.update({"mg_" + k: v for k, v in det.merged_detections()._asdict().items()})
    if det._pm_kw is not None:
        snap.update({"pm_" + k: v for k, v in det._pm_out._asdict().items()})
        snap.update({"tr_" + k: v for k, v in det._track_state._asdict().items()})
        snap.update({"tm_" + k: v for k, v in det._tm_state._asdict().items()})
        snap.update({"tm_" + k: v for k, v in det._tm_out._asdict().items()})
    return {k: v.detach().cpu().numpy().copy() for k, v in snap.items()}


def _restated_step(scan, tab, g, b, st, gate_map, seg_kw):
    """One sensor's scroll -> cast -> segments -> merge -> person motion -> tracks -> map -> track map on the step's own
    pose and NMS records; ``st``: the sensor's restated state, advanced in place.  -> {prefixed field: value}."""
    grid_scroll_oracle(g["trans"][b], st["grid"], st["origin"], st["base"], st["offset"], STREAM_RES, 64)
    nms = (g["nms_inst"][b], g["nms_num"][b], g["nms_cls"][b]) if "nms_inst" in g else (None, None, None)
    prim = (nms[0], nms[1], g["nms_xy"][b], nms[2]) if "nms_inst" in g else ()
    rot, trans = g["rot"][b], g["trans"][b]
    cast = grid_cast_oracle(scan, tab, rot, trans, st["grid"], st["origin"], STREAM_RES, *nms,
                            **dict(CAST_DEFAULTS, max_range=STREAM_RANGE))
    seg = novel_segments_oracle(scan, tab, cast["point_class"], *nms, **seg_kw)
    mg = merge_detections_oracle(seg["instance_mask"], seg["num_det"], seg["det_xy"], seg["det_cls"], *prim)
    pm = person_motion_oracle(scan, tab, mg["instance_mask"], mg["num_det"], mg["det_xy"], mg["det_cls"], rot, trans,
                              st["pm"])
    track_step(st["tr"], pm["det_xy_world"], pm["det_flow"], pm["det_valid"], mg["num_det"], mg["instance_mask"])
    by = (mg["instance_mask"], mg["num_det"], mg["det_cls"]) if gate_map else nms
    gm = grid_map_oracle(scan, tab, rot, trans, st["grid"], st["origin"], STREAM_RES, *by,
                         **dict(MAP_DEFAULTS, max_range=STREAM_RANGE))
    tm = track_map_oracle(mg["instance_mask"], mg["num_det"], gm["point_cell"], gm["point_prior"], gm["det_points"],
                          gm["det_free"], st["tr"]["track_id"], st["tr"]["track_state"], st["tr"]["track_det"], st["tm"],
                          **TM_DEFAULTS)
    want = {"point_class": cast["point_class"], "grid": st["grid"], "origin": st["origin"]}
    for prefix, rec in (("ns_", seg), ("mg_", mg), ("pm_", pm), ("tr_", st["tr"]), ("gm_", gm), ("tm_", tm),
                        ("tm_", st["tm"])):
        want.update({prefix + k: v for k, v in rec.items()})
    return want


@pytest.mark.parametrize("case", sorted(CASES))
def test_streaming_detector_eager_graph_and_restated_chain(case):
    from planar_optical_flow_amd.streaming import StreamingDetector
    from test_novel_segments_gpu import _stream_model, drives_with_a_walker
    ego, with_nms, gate_map = CASES[case]
    B, size, res, T = 2, STREAM_SIZE, STREAM_RES, 12
    scans, poses = drives_with_a_walker()
    model = _stream_model(13)
    seg_set = dict(jump=0.25, min_points=4)
    kw = dict(batch=B, cls_thresh=0.5, grid_map=dict(size=size, res=res, max_range=STREAM_RANGE),
              ego_motion=dict(method=ego), grid_scroll=dict(margin=64), grid_cast=dict(max_range=STREAM_RANGE),
              novel_segments=seg_set)
    if with_nms:
        kw.update(PERSON, nms_min_dist=0.5)
    mine = dict(kw, merge_detections=dict(gate_map=gate_map), **PERSON)
    eager = StreamingDetector(model, graph=False, **mine)
    graphed = StreamingDetector(model, graph=True, **mine)
    parent = StreamingDetector(model, graph=True, **kw)         # what the detector is without the stage
    assert parent._mg_kw is None and not any(n.startswith("_mg_") and n != "_mg_kw" for n in dir(parent))
    assert len(eager._stages) == len(parent._stages) + 1 + (0 if with_nms else len(PERSON))
    names = [s.launch.__name__ for s in graphed._stages]
    assert names == ["_keyframe_stage" if ego == "keyframe" else "_match_stage", "_grid_scroll_stage", "_grid_cast_stage",
                     "_novel_segments_stage", "_merge_stage", "_motion_stage", "_track_stage", "_grid_stage",
                     "_track_map_stage"] + (["_keep_scan"] if ego == "scan_match" else [])
    if with_nms:                                               # without the argument: today's table, in today's order
        assert [s.launch.__name__ for s in parent._stages] == \
            [names[0], "_grid_scroll_stage", "_motion_stage", "_track_stage", "_grid_cast_stage", "_novel_segments_stage",
             "_grid_stage", "_track_map_stage"] + names[9:]
    assert graphed._mg_kw == DEFAULTS and graphed._mg_gates is gate_map
    tab = graphed.tab.cpu().numpy()
    seg_kw = dict(SEG_DEFAULTS, **seg_set)
    half = 0.5 * res * size
    start = poses[0][:, :2]

    def run():
        sts = [dict(grid=np.zeros((size, size), np.int16), origin=start[b] - half, base=start[b] - half,
                    offset=np.zeros(2, np.int32), pm=motion_state(450), tr=new_track_state(STREAM_M, 450),
                    tm=new_tm_state(STREAM_M)) for b in range(B)]
        appended = absorbed = differs = 0
        first_appended = None
        for det in (eager, graphed, parent):
            det.reset(pose=poses[0])
        for t in range(T):
            for det in (eager, graphed, parent):
                if t == 0 and det is not parent:
                    with pytest.raises(RuntimeError, match="merge_detections"):
                        det.merged_detections()
                det(torch.from_numpy(scans[t]).cuda())
            e, g, p = _snapshot(eager), _snapshot(graphed), _snapshot(parent)
            for k in e:
                assert same_bits(e[k], g[k]), (t, k)           # eager and replayed: identical bits
            for b in range(B):
                want = _restated_step(scans[t, b], tab, g, b, sts[b], gate_map, seg_kw)
                for k, v in want.items():
                    got = g[k][b]
                    assert same_bits_nan(got, np.asarray(v, got.dtype).reshape(got.shape)), (t, b, k)
            counts = g["mg_merge_count"]
            if first_appended is None and counts[:, 1].any():
                first_appended = t
            appended, absorbed = appended + int(counts[:, 1].sum()), absorbed + int(counts[:, 2].sum())
            same = np.array_equal(p["grid"], g["grid"])
            if first_appended is None:                         # nothing appended yet: the detector without the argument
                for k in p:
                    assert same_bits(p[k], g[k]), (t, k)
            if not gate_map:
                assert same and same_bits(p["gm_point_prior"], g["gm_point_prior"]), t
            differs += not same
        rec = graphed.merged_detections()
        assert rec is graphed._mg_out and type(rec).__name__ == "MergedDetections"
        # the accessors answer per merged row
        num = g["mg_num_det"]
        per, _ = graphed.person_motion()
        live, det_track, _ = graphed.tracks()
        _, det_class, _, _ = graphed.track_map()
        for b in range(B):
            assert len(per[b]["valid"]) == len(det_track[b]) == len(det_class[b]) == num[b]
            assert same_bits(per[b]["dets_cls"], g["mg_det_cls"][b, :num[b]])
        if with_nms:
            dets, inst = graphed.detections()                  # stays the NMS's
            assert [len(d[1]) for d in dets] == g["nms_num"].tolist() and np.array_equal(inst, g["nms_inst"])
        tracked = int(sum((st["tr"]["track_id"] != 0).sum() for st in sts))
        return appended, absorbed, differs, first_appended, tracked

    result = run()
    print("%s: %d rows appended and %d absorbed over %d scans of %d sensors, the first at scan %s; the grid differs from "
          "the parent's after %d scans; %d live tracks at the end" % (case, result[0], result[1], T, B, result[3],
                                                                      result[2], result[4]))
    assert result[0] > 0                                       # the walker the net does not report becomes a row ...
    if with_nms:
        assert (result[2] > 0) == gate_map                     # ... and gated by the merged record the map is another
    assert graphed._graph is not None and eager._graph is None
    for det in (eager, graphed):
        det.reset(pose=(1.0, -2.0, 0.25))
        with pytest.raises(RuntimeError):
            det.merged_detections()
    assert run() == result                                     # the same sequence again behind a reset


def test_streaming_detector_constructor_rules():
    from planar_optical_flow_amd.streaming import StreamingDetector
    from test_novel_segments_gpu import _stream_model
    model = _stream_model(13)
    grid = dict(grid_map=dict(size=64))
    full = dict(grid, grid_cast=dict(), novel_segments=dict())
    with pytest.raises(ValueError, match="novel_segments missing"):
        StreamingDetector(model, merge_detections=dict(), grid_cast=dict(), **grid)
    with pytest.raises(ValueError, match="novel_segments and grid_cast and grid_map missing"):
        StreamingDetector(model, merge_detections=dict())
    with pytest.raises(ValueError, match="merge_detections with a flow_model is not built"):
        StreamingDetector(model, merge_detections=dict(), nms_min_dist=0.5, flow_model=torch.nn.Identity(), **full)
    with pytest.raises(ValueError, match="one gate"):
        StreamingDetector(model, merge_detections=dict(), **dict(full, novel_segments=dict(gate_map=True)))
    # the refusals of the detector without the argument keep their words
    with pytest.raises(ValueError, match="gate_map with nms_min_dist is not built"):
        StreamingDetector(model, nms_min_dist=0.5, **dict(full, novel_segments=dict(gate_map=True)))
    with pytest.raises(ValueError, match="person_motion needs nms_min_dist"):
        StreamingDetector(model, person_motion=dict(), **full)
    for bad in (dict(absorb_pct=-1), dict(absorb_pct=102)):
        with pytest.raises(ValueError, match="absorb_pct"):
            StreamingDetector(model, merge_detections=bad, **full)
    for bad in (dict(cls_thresh=0.5), dict(res=0.1), dict(absorb=1)):
        with pytest.raises(ValueError, match="unknown merge_detections settings"):
            StreamingDetector(model, merge_detections=bad, **full)
    plain = StreamingDetector(model, **full)
    assert plain._mg_kw is None and not any(name.startswith("_mg_") and name != "_mg_kw" for name in dir(plain))
    with pytest.raises(RuntimeError, match="merge_detections"):
        plain.merged_detections()
    # a pose per call, without the NMS: the detector-free chain; the first scan of a sequence runs the stage
    det = StreamingDetector(model, cls_thresh=0.3, merge_detections=dict(absorb_pct=101), person_motion=dict(),
                            tracks=dict(), **full)
    assert det._mg_kw == dict(cls_thresh=0.3, absorb_pct=101) and det._mg_gates
    det(torch.zeros(450).cuda() + 3.0, pose=(1.0, 2.0, 0.5))
    o = det.merged_detections()
    assert o is det._mg_out and not bool(o.num_det.any()) and o.merge_count.tolist() == [[0, 0, 0, 0]]
    assert (o.b_row == -1).all() and det.person_motion()[0][0]["valid"].shape == (0,)
