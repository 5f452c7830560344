"""Person motion without a flow net (pof_person_motion, N11) on the GPU: the device against the NumPy restatement of
tests/test_person_motion.py with the state carried on the device, every integer and every float output and state field
BIT FOR BIT (the arithmetic is IEEE basic operations in a stated order and contraction is off, so the derived tolerance
is zero; a NaN equals any NaN) -- at both kernel forms, at the largest scan, with every row a detection; at five batch
positions, in two runs and in two replays of a captured step; at the limits; through ``utils.PersonMotion``; and as the
tail of the streaming detector with the three sources of a pose, eager and replayed, chained with the tracker."""
import os
import sys

import numpy as np
import pytest
import torch

from test_person_motion import (DEFAULTS, OUT_FLOAT, OUT_INT, STATE_FIELDS, axis_table, motion_state, people_scene,
                                person_motion_oracle, rule_scans, same_bits, tie_scans)
from test_scan_match import angle_table, trajectory
from test_tracks import FLOAT_FIELDS as TRACK_FLOAT
from test_tracks import INT_FIELDS as TRACK_INT
from test_tracks import new_state as new_track_state, track_step

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "planar_optical_flow_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

FIELDS = OUT_FLOAT + OUT_INT
TRACK_TOL = 1e-12                                              # tests/test_tracks_gpu.py's bound on the track state


@pytest.fixture(scope="module")
def ops():
    from planar_optical_flow_amd import ops as _ops
    return _ops


def _inputs(scans, tab):
    """One step's inputs of B sensors (dicts of ranges, inst, num_det, det_xy, det_cls, rot, trans) as device tensors."""
    stack = lambda k, dt: torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(s[k]) for s in scans]), dtype=dt)).cuda()
    return (stack("ranges", np.float32), torch.from_numpy(np.asarray(tab, np.float64)).cuda(), stack("inst", np.int32),
            stack("num_det", np.int32), stack("det_xy", np.float64), stack("det_cls", np.float64),
            stack("rot", np.float32), stack("trans", np.float64))


def _host(out, state):
    h = {k: getattr(out, k).cpu().numpy() for k in FIELDS}
    h.update({k: getattr(state, k).cpu().numpy() for k in STATE_FIELDS})
    return h


def dev_steps(ops, seqs, tab, **kw):
    """The device's outputs and state after every step; seqs: one sequence per sensor, all of one length."""
    B, N = len(seqs), len(seqs[0][0]["ranges"])
    state, out, res = ops.person_motion_state(B, N), ops.person_motion_buffers(B, N), []
    for scans in zip(*seqs):
        ops.person_motion(*_inputs(scans, tab), state, out=out, **kw)
        res.append(_host(out, state))
    return res


def oracle_steps(seq, tab, **kw):
    state, res = motion_state(len(seq[0]["ranges"])), []
    for s in seq:
        o = person_motion_oracle(s["ranges"], tab, s["inst"], s["num_det"], s["det_xy"], s["det_cls"], s["rot"],
                                 s["trans"], state, **kw)
        o.update({k: v.copy() for k, v in state.items()})
        res.append(o)
    return res


def check_sequences(ops, seqs, tab, what, **kw):
    kw = dict(DEFAULTS, **kw)
    got = dev_steps(ops, seqs, tab, **kw)
    pairs = 0
    for b, seq in enumerate(seqs):
        for t, want in enumerate(oracle_steps(seq, tab, **kw)):
            for k in FIELDS + STATE_FIELDS:
                assert same_bits(got[t][k][b], np.asarray(want[k], got[t][k].dtype)), (what, b, t, k)
            pairs += int((want["det_prev"] >= 0).sum())
    print("%s: %d sensors x %d scans, %d pairs, every field the restatement's bits" % (what, len(seqs), len(seqs[0]), pairs))
    return got


def crowd_seq(N, T, n_det, seed, min_points=3):
    """n_det people on a circle of N beams around the sensor, person p on ``N // n_det`` consecutive beams at one of five
    radii, drifting radially by up to 0.3 m per scan (every 13th jumps 0.7 m in scan 2: beyond reach).  Every 7th is
    below the score threshold, every 11th has fewer than ``min_points`` points (when there are beams to spare); a
    twentieth of the beams is inf, NaN, at max_range or beyond it; a few beams carry ids that are nobody's.  The rows
    are permuted in every scan and the pose is fixed and not the identity.  -> (tab, list of scans)."""
    rng = np.random.default_rng(seed)
    tab = angle_table(N, 2.0 * np.pi / N)
    width = N // n_det
    radius = 5.0 + 2.5 * (np.arange(n_det) % 5) + rng.uniform(-0.2, 0.2, n_det)
    phi, t0 = rng.uniform(-np.pi, np.pi), rng.uniform(-2.0, 2.0, 2)
    rot = np.array([[np.cos(phi), -np.sin(phi)], [np.sin(phi), np.cos(phi)]]).astype(np.float32)
    scans = []
    for t in range(T):
        radius = radius + rng.uniform(-0.3, 0.3, n_det)
        if t == 2:
            radius[::13] += 0.7
        ranges, inst = np.full(N, 30.0), np.zeros(N, np.int32)
        det_xy, det_cls = np.zeros((N, 2)), np.zeros(N)
        row = rng.permutation(n_det)
        for p in range(n_det):
            n = min(min_points - 1, width) if p % 11 == 5 and width >= min_points else width
            beams = np.arange(p * width, p * width + n)
            ranges[beams] = radius[p] + rng.normal(0.0, 0.01, n)
            inst[beams] = row[p] + 1
            mid = p * width + width // 2
            det_xy[row[p]] = radius[p] * tab[N + 2 * mid:N + 2 * mid + 2] + rng.normal(0.0, 0.03, 2)
            det_cls[row[p]] = 0.2 if p % 7 == 3 else rng.uniform(0.6, 1.0)
        spoiled = rng.choice(N, N // 20, replace=False)
        ranges[spoiled] = rng.choice([np.inf, np.nan, 20.0, 25.0], len(spoiled))
        inst[rng.choice(N, 3, replace=False)] = [n_det + 1, -1, N + 5]
        scans.append(dict(ranges=ranges.astype(np.float32), inst=inst, num_det=np.int32(n_det), det_xy=det_xy,
                          det_cls=det_cls, rot=rot, trans=t0))
    return tab, scans


# ------------------------------------------------------------------ 1. the device against the restatement
def test_rooms_with_people_three_sensors(ops):
    scenes = [people_scene(seed, 5, 0.2) for seed in (21, 22, 23)]
    got = check_sequences(ops, [sc["scans"] for sc in scenes], scenes[0]["tab"], "N=450, B=3")
    for b, sc in enumerate(scenes):                            # and the scenario's truth, on the device's own output
        for t in range(1, 5):
            assert np.array_equal(got[t]["det_prev"][b][sc["rows"][t]], sc["rows"][t - 1])
    assert not np.array_equal(got[-1]["det_flow"][0], got[-1]["det_flow"][1])


@pytest.mark.parametrize("N", [512, 513])
def test_both_kernel_forms(ops, N):
    (tab, a), (_, b) = crowd_seq(N, 5, 40, seed=N), crowd_seq(N, 5, 40, seed=N + 1)
    got = check_sequences(ops, [a, b], tab, "N=%d, B=2" % N)
    prev = got[-1]["det_prev"][0][:40]
    assert (prev >= 0).sum() >= 20 and (prev < 0).sum() >= 5 and (got[2]["det_prev"][0][:40] < 0).sum() >= 8


def test_largest_scan_with_340_detections(ops):
    tab, seq = crowd_seq(4096, 5, 340, seed=7)
    got = check_sequences(ops, [seq], tab, "N=4096, 340 detections")
    assert (got[-1]["det_prev"][0] >= 0).sum() >= 100
    cand = got[-1]["prev_cand"][0][:340]
    assert 0 < (cand == 0).sum() < 340 and got[-1]["prev_num"][0] == 340
    assert (got[-1]["det_count"][0][:340] < 3).any() and (got[-1]["det_valid"][0][:340] == 0).any()


def test_every_row_of_a_64_beam_scan_its_own_detection(ops):
    tab, seq = crowd_seq(64, 6, 64, seed=9, min_points=1)
    got = check_sequences(ops, [seq, seq[::-1]], tab, "N=64, 64 detections", min_points=1, reach=1.0)
    assert got[-1]["prev_num"][0] == 64 and (got[-1]["det_count"][0] <= 1).all()
    assert (got[-1]["det_prev"][0] >= 0).sum() >= 20


def test_rules_and_ties_on_the_device(ops):
    tab = axis_table(64)
    for what, scans, kw in (("rules", rule_scans(), {}), ("rules, loose", rule_scans(), dict(min_points=1, cls_thresh=0.1)),
                            ("rules, far", rule_scans(), dict(reach=0.75)),
                            ("tie/previous rows", tie_scans()["previous rows"], {}),
                            ("tie/current rows", tie_scans()["current rows"], {})):
        got = check_sequences(ops, [[s.inputs() for s in scans]], tab, what, **dict(dict(min_points=2), **kw))
        if what == "rules":
            assert list(got[1]["det_prev"][0][:8]) == [-1, 0, -1, -1, -1, 4, -1, 5]
        if what == "tie/previous rows":
            assert got[1]["det_prev"][0][0] == 1
        if what == "tie/current rows":
            assert list(got[1]["det_prev"][0][:3]) == [-1, 0, -1]


# ------------------------------------------------------------------ 2. determinism and limits
def test_a_sensor_gives_the_same_bits_at_five_batch_positions_and_in_two_runs(ops):
    tab, a = crowd_seq(450, 5, 30, seed=31)
    others = [crowd_seq(450, 5, 30, seed=32 + i)[1] for i in range(3)]
    seqs = [a, others[0], a, others[1], a, others[2], a, a]
    first, again, alone = (dev_steps(ops, s, tab, **DEFAULTS) for s in (seqs, seqs, [a]))
    for t in range(5):
        for k in FIELDS + STATE_FIELDS:
            assert same_bits(first[t][k], again[t][k]), k
            for b in (0, 2, 4, 6, 7):
                assert same_bits(first[t][k][b], alone[t][k][0]), (k, b)
    assert not np.array_equal(first[-1]["det_centre"][0], first[-1]["det_centre"][1])


def test_two_replays_of_a_captured_step_with_a_reset_in_between(ops):
    tab, a = crowd_seq(513, 5, 30, seed=41)
    _, b = crowd_seq(513, 5, 30, seed=42)
    seqs = [a, b]
    want = dev_steps(ops, seqs, tab, **DEFAULTS)
    bufs = [torch.zeros_like(t) for t in _inputs([s[0] for s in seqs], tab)]
    state, out = ops.person_motion_state(2, 513), ops.person_motion_buffers(2, 513)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.person_motion(*bufs, ops.person_motion_state(2, 513), **DEFAULTS)  # warm-up on a state of its own
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.person_motion(*bufs, state, out=out, **DEFAULTS)
    for _ in range(2):
        ops.person_motion_reset(state)
        for t in range(5):
            for dst, src in zip(bufs, _inputs([s[t] for s in seqs], tab)):
                dst.copy_(src)
            graph.replay()
            got = _host(out, state)
            for k in FIELDS + STATE_FIELDS:
                assert same_bits(got[k], want[t][k]), (t, k)
    assert int(state.prev_num[0]) == 30


def test_refused_calls_leave_state_and_outputs_untouched(ops):
    from planar_optical_flow_amd._lib import POF_E_SHAPE, PofError
    for N, kw, error in ((4097, {}, PofError), (64, dict(min_points=0), AssertionError), (64, dict(reach=-1.0), AssertionError)):
        tab, seq = crowd_seq(N, 1, 8, seed=5)
        state, out = ops.person_motion_state(1, N), ops.person_motion_buffers(1, N)
        for t in tuple(state) + tuple(out):                    # sentinels
            t.copy_(torch.from_numpy(np.random.default_rng(1).integers(1, 100, tuple(t.shape))).to(t.dtype))
        before = _host(out, state)
        with pytest.raises(error) as e:
            ops.person_motion(*_inputs(seq[:1], tab), state, out=out, **dict(DEFAULTS, **kw))
        if error is PofError:
            assert e.value.code == POF_E_SHAPE
        after = _host(out, state)
        assert all(same_bits(before[k], after[k]) for k in before)
    tab, seq = crowd_seq(64, 1, 8, seed=5)
    with pytest.raises(ValueError):
        ops.person_motion(*_inputs(seq[:1], tab), ops.person_motion_state(1, 65))
    with pytest.raises(ValueError):
        ops.person_motion(*_inputs(seq[:1], tab), ops.person_motion_state(1, 64), out=ops.person_motion_buffers(2, 64))
    ins = _inputs(seq[:1], tab)
    empty = ops.person_motion(ins[0][:0], ins[1], *(t[:0] for t in ins[2:]), ops.person_motion_state(0, 64))
    assert empty.det_flow.shape == (0, 64, 2)
    state = ops.person_motion_state(1, 64)
    ops.person_motion(*_inputs(seq[:1], tab), state)
    assert int(state.prev_num[0]) == 8 and ops.person_motion_reset(state) is not None
    assert not any(t.any() for t in state)


# ------------------------------------------------------------------ 3. the reference-shaped wrapper
def test_person_motion_wrapper_equals_the_direct_calls(ops):
    import src.utils.utils as u
    scene = people_scene(24, 3, 0.2)
    N = 450
    phi = scene["tab"][:N]
    rng = np.random.default_rng(3)
    pm = u.PersonMotion(phi, reach=0.6, min_dist=0.5)
    tracker = u.PersonTracker(max_tracks=64)
    tab = u._table_for(phi)
    state = ops.person_motion_state(1, N)
    paired = 0
    cls, reg = rng.uniform(0.05, 0.95, (N, 1)), rng.normal(0.0, 0.05, (N, 2))  # the same "net output" for every scan
    for t, s in enumerate(scene["scans"]):
        res = pm.update(s["ranges"], cls, reg, scene["poses"][t])
        ranges = torch.from_numpy(s["ranges"]).cuda().reshape(1, N)
        xy, dc, num, inst = ops.nms_predicted_center(ranges, tab, torch.from_numpy(cls[:, 0].copy()).cuda().reshape(1, N),
                                                     torch.from_numpy(reg).cuda().reshape(1, N, 2), 0.5)
        rot, trans, _ = u._pose_terms(scene["poses"][t][None])
        o = ops.person_motion(ranges, tab, inst, num, xy, dc, torch.from_numpy(rot).cuda(), torch.from_numpy(trans).cuda(),
                              state, reach=0.6)
        m = int(num[0])
        for key, field in (("dets_xy_world", "det_xy_world"), ("person_flow", "det_flow"), ("centre", "det_centre"),
                           ("count", "det_count"), ("prev", "det_prev")):
            assert same_bits(res[key], getattr(o, field)[0, :m].cpu().numpy()), key
        assert np.array_equal(res["valid"], o.det_valid[0, :m].cpu().numpy().astype(bool)) and res["valid"].dtype == bool
        assert np.array_equal(res["dets_cls"][:, 0], dc[0, :m].cpu().numpy()) and res["dets_cls"].shape == (m, 1)
        assert np.array_equal(res["instance_mask"], inst[0].cpu().numpy())
        paired += int((res["prev"] >= 0).sum())
        ids, tracks = tracker.update(res)                      # the tracker takes the dict as it is
        assert len(ids) == m and len(tracks["id"]) > 0
    assert paired > 0
    pm.reset()
    res = pm.update(scene["scans"][0]["ranges"], cls, reg)
    assert (res["prev"] == -1).all() and np.isnan(res["person_flow"]).all()
    with pytest.raises(ValueError):
        u.PersonMotion(phi, reaches=1.0)


# ------------------------------------------------------------------ 4. streaming detector
def _stream_model(seed):
    from planar_optical_flow_amd.src.depracted.model.dr_spaam import SpatialDROW
    torch.manual_seed(seed)
    return SpatialDROW(num_scans=5, num_pts=56, alpha=0.5, window_size=11, pedestrian_only=True).cuda().eval()


def _detector_snapshot(det):
    """Everything a step leaves behind, on the host."""
    xy, conf, num, inst = det._dets
    snap = {"pred_cls": det.pred_cls, "pred_reg": det.pred_reg, "det_xy": xy, "det_cls": conf, "num_det": num, "inst": inst,
            "rot": det._pose_rot, "trans": det._pose_trans}
    snap.update({k: getattr(det._pm_out, k) for k in FIELDS})
    snap.update({k: getattr(det._pm_state, k) for k in STATE_FIELDS})
    snap.update({k: getattr(det._track_state, k) for k in det._track_state._fields})
    return {k: v.detach().cpu().numpy().copy() for k, v in snap.items()}


@pytest.mark.parametrize("ego", ["keyframe", "scan_match", None])
def test_streaming_detector_eager_graph_and_restatement(ego):
    from planar_optical_flow_amd.streaming import StreamingDetector
    B, T, N = 2, 6, 450
    scans, poses = trajectory(T, B, seed=71, noise=0.01)
    model = _stream_model(13)
    kw = dict(batch=B, nms_min_dist=0.5, cls_thresh=0.0, person_motion=dict(), tracks=dict())
    if ego is not None:
        kw["ego_motion"] = dict(method=ego)
    eager, graphed = StreamingDetector(model, graph=False, **kw), StreamingDetector(model, graph=True, **kw)
    tab = graphed.tab.cpu().numpy()
    M = graphed._track_state.track_id.shape[1]

    def run():
        pm_states = [motion_state(N) for _ in range(B)]
        tr_states = [new_track_state(M, N) for _ in range(B)]
        pairs, ids = 0, []
        for t in range(T):
            for det in (eager, graphed):
                with pytest.raises(RuntimeError):
                    det.tracks() if t == 1 else det.person_motion() if t == 0 else det.person_flow()
                det(torch.from_numpy(scans[t]).cuda(), **({} if ego is not None else dict(pose=poses[t])))
            e, g = _detector_snapshot(eager), _detector_snapshot(graphed)
            for k in e:
                assert same_bits(e[k], g[k]), (t, k)           # eager and replayed: identical bits, state and tracks
            for b in range(B):
                want = person_motion_oracle(scans[t, b], tab, g["inst"][b], g["num_det"][b], g["det_xy"][b],
                                            g["det_cls"][b], g["rot"][b], g["trans"][b], pm_states[b],
                                            **dict(DEFAULTS, cls_thresh=0.0))
                want.update(pm_states[b])
                for k in FIELDS + STATE_FIELDS:
                    assert same_bits(g[k][b], np.asarray(want[k], g[k].dtype)), (t, b, k)
                track_step(tr_states[b], want["det_xy_world"], want["det_flow"], want["det_valid"], g["num_det"][b],
                           g["inst"][b])
                for k in TRACK_INT:
                    assert np.array_equal(g[k][b], tr_states[b][k]), (t, b, k)
                for k in TRACK_FLOAT:
                    assert np.abs(g[k][b] - tr_states[b][k]).max(initial=0.0) <= TRACK_TOL, (t, b, k)
                pairs += int((want["det_prev"] >= 0).sum())
            dicts, dev = graphed.person_motion()
            assert dev is graphed._pm_out and len(dicts) == B
            for b, d in enumerate(dicts):
                m = int(g["num_det"][b])
                assert set(d) == {"dets_xy_world", "dets_cls", "person_flow", "count", "valid", "centre", "prev"}
                assert same_bits(d["person_flow"], g["det_flow"][b, :m]) and same_bits(d["centre"], g["det_centre"][b, :m])
                assert np.array_equal(d["prev"], g["det_prev"][b, :m]) and d["valid"].dtype == bool
            if t == 0:
                assert all(np.isnan(d["person_flow"]).all() and len(d["prev"]) > 0 for d in dicts)
            else:
                live, det_track, _ = graphed.tracks()
                ids.append([sorted(tr["id"] for tr in l) for l in live])
                assert all(len(dt) == int(g["num_det"][b]) for b, dt in enumerate(det_track))
            if ego is None:                                    # the pose that was given is the frame
                assert np.array_equal(g["trans"], poses[t][:, :2])
        return pairs, ids

    pairs, ids = run()
    print("ego=%s: %d pairs over %d scans of %d sensors" % (ego, pairs, T, B))
    assert pairs > 0 and graphed._graph is not None and eager._graph is None
    assert min(min(i) for i in ids[0]) == 1
    for det in (eager, graphed):
        det.reset()
        assert int(det._track_state.next_id.max()) == 1 and not det._track_state.track_id.any()
        assert not any(t.any() for t in det._pm_state)
        with pytest.raises(RuntimeError):
            det.person_motion()
    again = run()                                              # the same sequence again: ids restart at 1
    assert again == (pairs, ids)


def test_streaming_detector_constructor_rules():
    from planar_optical_flow_amd.streaming import StreamingDetector
    model = _stream_model(13)
    stub = torch.nn.Identity()
    with pytest.raises(ValueError):
        StreamingDetector(model, nms_min_dist=0.5, flow_model=stub, person_motion=dict())
    with pytest.raises(ValueError):
        StreamingDetector(model, person_motion=dict())                            # needs nms_min_dist
    with pytest.raises(ValueError):
        StreamingDetector(model, nms_min_dist=0.5, person_motion=dict(reaches=1.0))
    with pytest.raises(ValueError):
        StreamingDetector(model, nms_min_dist=0.5, person_motion=dict(min_points=0))
    with pytest.raises(ValueError):
        StreamingDetector(model, nms_min_dist=0.5, tracks=dict())                 # neither flow_model nor person_motion
    plain = StreamingDetector(model, nms_min_dist=0.5)
    with pytest.raises(ValueError):
        plain(torch.zeros(450).cuda() + 5.0, pose=(0.0, 0.0, 0.0))                # pose without flow_model / person_motion
    for name in ("_pm_out", "_pm_state", "_pm_no_ok", "_pose_dev", "_pose_host", "_track_state"):
        assert not hasattr(plain, name), name                                     # none of the new buffers
    assert plain._pm_kw is None
    matched = StreamingDetector(model, nms_min_dist=0.5, ego_motion=dict(method="scan_match"))
    assert not hasattr(matched, "_pm_out") and not hasattr(matched, "_pose_dev")
    with_pm = StreamingDetector(model, nms_min_dist=0.5, person_motion=dict(reach=0.4))
    assert with_pm._pm_out.det_flow.shape == (1, 450, 2) and with_pm._pm_kw["reach"] == 0.4
    assert not hasattr(with_pm, "_track_state") and not hasattr(with_pm, "_pm_no_ok")
    with_pm(torch.zeros(450).cuda() + 5.0, pose=(1.0, 2.0, 0.5))
    assert with_pm.person_motion()[1] is with_pm._pm_out
    with pytest.raises(RuntimeError):
        with_pm.person_flow()
    with pytest.raises(RuntimeError):
        with_pm.tracks()
    with pytest.raises(ValueError):
        StreamingDetector(model, nms_min_dist=0.5, ego_motion=dict(method="keyframe"), person_motion=dict())(
            torch.zeros(450).cuda() + 5.0, pose=(0.0, 0.0, 0.0))                  # a dead-reckoning detector takes no pose
