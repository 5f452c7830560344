"""Scan-to-grid matching (pof_grid_match, N13) on the GPU: the device against the NumPy restatement of
tests/test_grid_match.py, BIT FOR BIT -- scores, best, score, votes, ok, moved, correction, pose and trans; rot, which a
moved pose is written with through sincos, to one float32 ulp as tests/test_ego_motion_gpu.py holds pof_pose_advance's
(and to its incoming bits without ``moved``).  The grids are built on the CPU by ``grid_map_oracle`` and uploaded.  The
rule scenes, every shape of ``device_cases``, five batch positions and two runs, refused calls, ``utils.OccupancyGrid.
localize``, and the stage of the streaming detector, eager and replayed.

The streaming test spoils a scan with 25 m on every beam -- no return inside max_range, so both scan pairs around it
fail and no point votes -- and not with NaN: a NaN scan would also run through the network and stay in its template."""
import os
import sys

import numpy as np
import pytest
import torch

from test_grid_map import grid_map_oracle
from test_grid_match import (CELL, DEFAULTS, OUT_DTYPES, OUT_FIELDS, device_cases, drive, grid_match_oracle, room_case,
                             rule_cases, run_case)

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "planar_optical_flow_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

EXACT = OUT_FIELDS + ("pose", "trans")


@pytest.fixture(scope="module")
def ops():
    from planar_optical_flow_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def cases():
    return device_cases()


def _cuda(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def _inputs(ops, case, sensors):
    """-> (ranges, tab, rot, trans, pose, state) on the device and the NMS keywords."""
    stack = lambda k, dt: _cuda(np.stack([np.asarray(s[k]) for s in sensors]), dt)
    nms = {}
    if "inst" in sensors[0]:
        nms = dict(instance_mask=stack("inst", np.int32), num_det=stack("num_det", np.int32),
                   det_cls=stack("det_cls", np.float64))
    state = ops.GridMapState(stack("grid", np.int16), stack("origin", np.float64))
    return (stack("ranges", np.float32), _cuda(case["tab"], np.float64), stack("rot", np.float32),
            stack("trans", np.float64), stack("pose", np.float64), state), nms


def dev_case(ops, case, sensors=None):
    """The device's outputs and pose terms for the sensors of a case in one batch, on the host."""
    sensors = case["sensors"] if sensors is None else sensors
    args, nms = _inputs(ops, case, sensors)
    grid = args[5].grid.clone()
    out = ops.grid_match(*args, res=case["res"], **nms, **case["kw"])
    got = {k: getattr(out, k).cpu().numpy() for k in OUT_FIELDS}
    got.update(rot=args[2].cpu().numpy().reshape(len(sensors), 4), trans=args[3].cpu().numpy(), pose=args[4].cpu().numpy())
    assert torch.equal(grid, args[5].grid)                     # the grid is read only
    return got


def assert_equal(got, b, want, sensor, what):
    for k, dt in zip(OUT_FIELDS, OUT_DTYPES):
        assert got[k].dtype == dt and np.array_equal(got[k][b], want[k]), (what, b, k)
    assert got["pose"][b].tobytes() == want["pose"].tobytes() and got["trans"][b].tobytes() == want["trans"].tobytes(), (what, b)
    if want["moved"]:
        assert np.all(np.abs(got["rot"][b] - want["rot"]) <= np.spacing(np.abs(want["rot"]))), (what, b)   # one float32 ulp
    else:
        assert got["rot"][b].tobytes() == np.asarray(sensor["rot"], np.float32).tobytes(), (what, b)


def check_case(ops, case, what):
    got, want = dev_case(ops, case), run_case(case)
    for b, (s, w) in enumerate(zip(case["sensors"], want)):
        assert_equal(got, b, w, s, what)
    print("%s: %d sensors, scores %s, votes %s, moved %s: every output the restatement's bits"
          % (what, len(want), got["scores"].shape[1:], got["votes"].tolist(), got["moved"].tolist()))
    return got


# ------------------------------------------------------------------ 1. the device against the restatement
@pytest.mark.parametrize("name", sorted(rule_cases()))
def test_rule_scenes(ops, name):
    check_case(ops, rule_cases()[name], name)


@pytest.mark.parametrize("name", sorted(device_cases()))
def test_shapes(ops, cases, name):
    got = check_case(ops, cases[name], name)
    assert got["scores"].any()
    if name in ("128 x 192 with people", "N 512", "N 513", "no NMS", "largest search"):
        assert got["moved"].any()


# ------------------------------------------------------------------ 2. determinism
def test_same_bits_at_five_batch_positions_and_in_two_runs(ops, cases):
    case = cases["128 x 192 with people"]
    me, other = case["sensors"][0], room_case(61, 450, 128, 192, offsets=((-0.2, 0.1, 0.01),))["sensors"][0]
    want = run_case(dict(case, sensors=[me]))[0]
    runs = []
    for pos in list(range(5)) + [2]:
        sensors = [other] * 5
        sensors[pos] = me
        got = dev_case(ops, case, sensors)
        assert_equal(got, pos, want, me, pos)
        runs.append(got)
    for k in EXACT + ("rot",):                                 # the two runs at position 2: every sensor's bits
        assert runs[2][k].tobytes() == runs[5][k].tobytes(), k


# ------------------------------------------------------------------ 3. refused calls
def test_refused_calls_leave_outputs_and_pose_terms_untouched(ops):
    from planar_optical_flow_amd import _lib
    from planar_optical_flow_amd._lib import POF_E_BADARG, POF_E_SHAPE, PofError
    rng = np.random.default_rng(1)
    lib = _lib.load()
    ptr = lambda t: None if t is None else t.data_ptr()

    def sentinel_call(N, kw, drop=()):
        """The raw entry point on sentinel-filled outputs and pose terms -> (status, everything untouched)."""
        v = dict(dict(DEFAULTS, res=0.1), **kw)
        case = room_case(5, min(N, 64), 64, 64)
        (ranges, tab, rot, trans, pose, state), nms = _inputs(ops, case, case["sensors"])
        if N > 64:
            ranges, tab = torch.ones(1, N, device="cuda"), torch.zeros(3 * N, dtype=torch.float64, device="cuda")
            nms = {k: torch.zeros((1, N), dtype=t.dtype, device="cuda") if t.dim() == 2 else t for k, t in nms.items()}
        K, T = max(min(v["rotations"], 33), 1), 2 * max(min(v["reach"], 16), 0) + 1
        out = ops.GridMatch(*(torch.zeros(shape, dtype=dt, device="cuda") for (dt, _), shape in
                              zip(ops.GridMatch.spec, ops._shapes_of(ops.GridMatch, B=1, K=K, T=T))))
        table = ops.grid_match_table(0.01, K if K % 2 else K + 1)
        watched = (rot, trans, pose) + tuple(out)
        for t in watched:
            t.copy_(torch.from_numpy(rng.integers(1, 100, tuple(t.shape))).to(t.dtype))
        before = [t.cpu().numpy() for t in watched]
        gate = [None if k in drop else ptr(nms[k]) for k in ("instance_mask", "num_det", "det_cls")]
        rc = lib.pof_grid_match(ptr(ranges), ptr(tab), *gate, v["cls_thresh"], v["max_range"], ptr(state.grid),
                                ptr(state.origin), v["res"], ptr(table), v["reach"], v["rotations"], v["min_points"],
                                v["min_score"], v["min_gain"], 1, N, 64, 64, ptr(pose), ptr(rot), ptr(trans),
                                *[ptr(t) for t in out], None)
        torch.cuda.synchronize()
        return rc, all(np.array_equal(a, t.cpu().numpy()) for a, t in zip(before, watched))

    assert sentinel_call(4097, {}) == (POF_E_SHAPE, True)
    for kw in (dict(rotations=8), dict(rotations=35), dict(reach=17), dict(res=0.0), dict(min_points=-1),
               dict(min_score=-1), dict(min_gain=-1), dict(max_range=0.0)):
        assert sentinel_call(64, kw) == (POF_E_BADARG, True), kw
    for drop in (("num_det",), ("instance_mask",), ("num_det", "det_cls")):
        assert sentinel_call(64, {}, drop) == (POF_E_BADARG, True), drop
    # the wrapper: the same refusals as exceptions, and its own shape checks
    case = room_case(5, 64, 64, 64, offsets=((0.2, -0.1, 0.0),), min_points=5, min_score=5)
    args, nms = _inputs(ops, case, case["sensors"])
    for kw, error in ((dict(rotations=8), ValueError), (dict(rotations=35), ValueError), (dict(reach=17), ValueError),
                      (dict(res=0.0), AssertionError), (dict(min_gain=-1), AssertionError)):
        with pytest.raises(error):
            ops.grid_match(*args, **dict(dict(res=0.1), **kw), **nms)
    with pytest.raises(PofError) as e:
        ops.grid_match(torch.ones(1, 4097, device="cuda"), torch.zeros(3 * 4097, dtype=torch.float64, device="cuda"),
                       *args[2:], res=0.1)
    assert e.value.code == POF_E_SHAPE
    for part in (("instance_mask",), ("num_det", "det_cls"), ("instance_mask", "det_cls")):
        with pytest.raises(ValueError):
            ops.grid_match(*args, res=0.1, **{k: nms[k] for k in part})
    with pytest.raises(ValueError):
        ops.grid_match(*args, res=0.1, out=ops.grid_match_buffers(1, 3, 9))               # buffers of another search
    with pytest.raises(ValueError):
        ops.grid_match(*args, res=0.1, table=ops.grid_match_table(0.01, 7))
    with pytest.raises(ValueError):
        ops.grid_match(*args[:4], torch.zeros(2, 3, dtype=torch.float64, device="cuda"), args[5], res=0.1)
    empty = ops.grid_match(args[0][:0], args[1], args[2][:0], args[3][:0], args[4][:0], ops.grid_map_state(0, 64, 64), res=0.1)
    assert empty.scores.shape == (0, 9, 9, 9)
    # the next good call works
    check_case(ops, case, "after the refusals")


# ------------------------------------------------------------------ 4. the reference-shaped wrapper
def test_occupancy_grid_localize_equals_the_direct_call(ops):
    import src.utils.utils as u
    tab_np, scans, truth = drive(21, spoil=False)
    N, res, size = 450, CELL, (128, 192)
    phi = tab_np[:N]
    og = u.OccupancyGrid(phi, res=res, size=size, max_range=10.0)
    rng = np.random.default_rng(3)
    cls, reg = rng.uniform(0.05, 0.3, (N, 1)), rng.normal(0.0, 0.05, (N, 2))
    cls[100:115], cls[300:310] = 0.9, 0.8                      # two people; everything else stays under cls_thresh
    for t in range(6):
        og.update(scans[t], truth[t])
    before = og.logodds.copy()
    tab = u._table_for(phi)
    state = ops.GridMapState(_cuda(before[None], np.int16), _cuda(og.origin[None], np.float64))
    moved = 0
    for gated, off, kw in ((False, (0.0, 0.0, 0.0), {}), (True, (0.21, -0.12, 0.02), {}),
                           (False, (-0.3, 0.3, -0.01), dict(reach=6, rotations=5, rot_step=0.02, min_gain=4))):
        odom = truth[6] + np.asarray(off)
        new, info = og.localize(scans[6], odom, *((cls, reg) if gated else ()), **kw)
        ranges = _cuda(scans[6][None], np.float32)
        nms = {}
        if gated:
            _, dc, num, inst = ops.nms_predicted_center(ranges, tab, _cuda(cls[:, 0][None], np.float64),
                                                        _cuda(reg[None], np.float64), 0.5)
            nms = dict(instance_mask=inst, num_det=num, det_cls=dc)
        rot, trans, _ = u._pose_terms(odom[None])
        pose = _cuda(odom[None], np.float64)
        o = ops.grid_match(ranges, tab, _cuda(rot, np.float32), _cuda(trans, np.float64), pose, state, res=res,
                           max_range=10.0, **nms, **kw)
        assert new.tobytes() == pose[0].cpu().numpy().tobytes()
        for k in ("best", "score", "correction"):
            assert np.array_equal(info[k], getattr(o, k)[0].cpu().numpy()), k
        assert (info["votes"], info["ok"], info["moved"]) == (int(o.votes[0]), bool(o.ok[0]), bool(o.moved[0]))
        assert info["moved"] == (off != (0.0, 0.0, 0.0)) and info["ok"] and (info["votes"] < 440) == gated
        if info["moved"]:
            left = np.asarray(off) + info["correction"]
            assert np.abs(left[:2]).max() <= res and np.array_equal(new, odom + info["correction"])
        moved += info["moved"]
    assert moved == 2 and np.array_equal(og.logodds, before)   # localize does not update the grid
    with pytest.raises(ValueError):
        og.localize(scans[6], truth[6], res=0.2)
    with pytest.raises(ValueError):
        og.localize(scans[6], truth[6], reaches=3)


# ------------------------------------------------------------------ 5. streaming detector
def _stream_model(seed):
    from planar_optical_flow_amd.src.depracted.model.dr_spaam import SpatialDROW
    torch.manual_seed(seed)
    return SpatialDROW(num_scans=5, num_pts=56, alpha=0.5, window_size=11, pedestrian_only=True).cuda().eval()


STREAM_T, STREAM_SPOILED = 8, 4


def _stream_scans(B):
    """[T,B,450]: ``drive``'s sensors, scan STREAM_SPOILED of every one without a return (25 m on every beam)."""
    scans = np.stack([drive(31 + b, spoil=False)[1][:STREAM_T] for b in range(B)], axis=1)
    scans[STREAM_SPOILED] = 25.0
    return scans, drive(31, spoil=False)[0]


def _snapshot(det, matched=True):
    """Everything the stage reads and leaves behind, on the host."""
    _, conf, num, inst = det._dets
    state, _ = det.grid_map()
    snap = {"det_cls": conf, "num_det": num, "inst": inst, "rot": det._pose_rot, "trans": det._pose_trans,
            "pose": det._pose_state, "grid": state.grid, "origin": state.origin}
    if matched:
        snap.update({k: getattr(det.grid_match()[1], k) for k in OUT_FIELDS})
    return {k: v.detach().cpu().numpy().copy() for k, v in snap.items()}


@pytest.mark.parametrize("tail", [False, True])
def test_streaming_detector_eager_graph_and_restatement(tail):
    from planar_optical_flow_amd.streaming import StreamingDetector
    B, N, size = 2, 450, 128
    scans, tab_np = _stream_scans(B)
    model = _stream_model(13)
    kw = dict(batch=B, nms_min_dist=0.5, cls_thresh=0.5, ego_motion=dict(method="scan_match"), grid_map=dict(size=size),
              angle_inc=float(tab_np[1] - tab_np[0]))
    if tail:
        kw.update(person_motion=dict(), tracks=dict())
    eager = StreamingDetector(model, graph=False, grid_match=dict(), **kw)
    graphed = StreamingDetector(model, graph=True, grid_match=dict(), **kw)
    parent = StreamingDetector(model, graph=True, **kw)       # the detector as it was: no grid_match
    assert parent._sg_kw is None and not hasattr(parent, "_sg_out") and not hasattr(parent, "_sg_table")
    assert len(graphed._stages) == len(parent._stages) + 1
    tab = graphed.tab.cpu().numpy()
    begin = (0.213, -0.127, 0.3)

    def run():
        grids = [np.zeros((size, size), np.int16) for _ in range(B)]
        for det in (eager, graphed, parent):
            det.reset(pose=begin)
        fired, history = [], []
        for t in range(STREAM_T):
            for det in (eager, graphed, parent):
                if t == 0 and det is not parent:
                    with pytest.raises(RuntimeError):
                        det.grid_match()
                det(torch.from_numpy(scans[t]).cuda())
            e, g = _snapshot(eager), _snapshot(graphed)
            for k in e:
                assert e[k].tobytes() == g[k].tobytes(), (t, k)    # eager and replayed: identical bits
            history.append(g)
            if t <= STREAM_SPOILED:                                # until something moves, the parent's bits
                p = _snapshot(parent, matched=False)
                assert not g["moved"].any() and all(p[k].tobytes() == g[k].tobytes() for k in p), t
            dicts, rec = graphed.grid_match()
            assert rec is graphed._sg_out and len(dicts) == B
            for b in range(B):
                assert dicts[b]["moved"] == bool(g["moved"][b]) and dicts[b]["votes"] == int(g["votes"][b])
                assert np.array_equal(dicts[b]["correction"], g["correction"][b])
            fired.append(g["moved"].astype(bool).tolist())
        return fired, history

    fired, history = run()
    print("tail=%s: moved per scan %s" % (tail, fired))
    assert all(fired[STREAM_SPOILED + 1]) and not any(any(f) for f in fired[:STREAM_SPOILED + 1])
    assert graphed._graph is not None and eager._graph is None
    again_fired, again = run()                                 # reset() in between: the same bits once more
    assert again_fired == fired
    for a, b in zip(history, again):
        assert all(a[k].tobytes() == b[k].tobytes() for k in a)


def test_streaming_step_equals_the_restatement():
    """The stage's launch on the detector's own buffers, held to the restatement on the step's own NMS results and
    incoming pose terms: the detector is stepped eagerly with the stage's incoming terms read back in front of it."""
    from planar_optical_flow_amd.streaming import StreamingDetector
    B, size = 2, 128
    scans, tab_np = _stream_scans(B)
    det = StreamingDetector(_stream_model(13), graph=False, batch=B, nms_min_dist=0.5, cls_thresh=0.5,
                            ego_motion=dict(method="scan_match"), grid_map=dict(size=size), grid_match=dict(),
                            angle_inc=float(tab_np[1] - tab_np[0]))
    det.reset(pose=(0.213, -0.127, 0.3))
    tab = det.tab.cpu().numpy()
    incoming = {}
    launch = det._grid_match_stage

    def recording(first):
        incoming.update(rot=det._pose_rot.cpu().numpy().copy(), trans=det._pose_trans.cpu().numpy().copy(),
                        pose=det._pose_state.cpu().numpy().copy(), grid=det._gm_state.grid.cpu().numpy().copy())
        launch(first)

    det._stages = tuple(s._replace(launch=recording) if s.launch == launch else s for s in det._stages)
    moved = 0
    for t in range(STREAM_T):
        det(torch.from_numpy(scans[t]).cuda())
        g = _snapshot(det)
        for b in range(B):
            want = grid_match_oracle(scans[t, b], tab, incoming["rot"][b], incoming["trans"][b], incoming["pose"][b],
                                     incoming["grid"][b], g["origin"][b], 0.1, g["inst"][b], g["num_det"][b],
                                     g["det_cls"][b], **DEFAULTS)
            got = {k: g[k] for k in OUT_FIELDS + ("pose", "trans")}
            got["rot"] = g["rot"].reshape(B, 4)
            assert_equal(got, b, want, dict(rot=incoming["rot"][b]), t)
            moved += int(want["moved"])
            # the scan went into the map at the corrected pose
            grid = incoming["grid"][b].copy()
            grid_map_oracle(scans[t, b], tab, g["rot"][b], g["trans"][b], grid, g["origin"][b], 0.1, g["inst"][b],
                            g["num_det"][b], g["det_cls"][b])
            assert np.array_equal(grid, g["grid"][b]), (t, b)
    assert moved >= B


def test_streaming_detector_constructor_rules():
    from planar_optical_flow_amd.streaming import StreamingDetector
    model = _stream_model(13)

    class DiffFlow(torch.nn.Module):
        def forward(self, prev, cur):
            return torch.cat([cur - prev, prev - cur], dim=2)

    match = dict(method="scan_match")
    for bad in (dict(grid_map=dict(size=64)),                                             # a pose per call
                dict(ego_motion=match),                                                   # no grid to match against
                dict(ego_motion=dict(method="keyframe"), grid_map=dict(size=64)),
                dict(ego_motion=dict(method="keyframe_map"), grid_map=dict(size=64)),
                dict(ego_motion=match, grid_map=dict(size=64), nms_min_dist=0.5, flow_model=DiffFlow()),
                dict(ego_motion=dict(), grid_map=dict(size=64), nms_min_dist=0.5, flow_model=DiffFlow())):
        with pytest.raises(ValueError):
            StreamingDetector(model, grid_match=dict(), **bad)
    for bad in (dict(reach=17), dict(rotations=8), dict(rotations=35), dict(min_gain=-1), dict(cls_thresh=0.5),
                dict(res=0.1), dict(reaches=4)):
        with pytest.raises(ValueError):
            StreamingDetector(model, ego_motion=match, grid_map=dict(size=64), grid_match=bad)
    plain = StreamingDetector(model, ego_motion=match, grid_map=dict(size=64))
    assert plain._sg_kw is None and not any(name.startswith("_sg_") and name != "_sg_kw" for name in dir(plain))
    with pytest.raises(RuntimeError):
        plain.grid_match()
    det = StreamingDetector(model, ego_motion=match, grid_map=dict(size=(64, 128), res=0.125),
                            grid_match=dict(reach=2, rotations=3, rot_step=0.02, min_points=10))
    assert det._sg_out.scores.shape == (1, 3, 5, 5) and det._sg_table.shape == (3, 3) and det._sg_kw["min_points"] == 10
    assert det._sg_table[1].tolist() == [0.0, 1.0, 0.0]
    # directly behind the scan matcher's stage
    names = [s.launch.__name__ for s in det._stages]
    assert names == ["_match_stage", "_grid_match_stage", "_grid_stage", "_keep_scan"]
    det(torch.zeros(450).cuda() + 3.0)
    dicts, rec = det.grid_match()
    assert rec is det._sg_out and dicts[0]["ok"] is False and dicts[0]["moved"] is False     # an empty grid scores 0
    assert dicts[0]["votes"] == 450 and not rec.scores.any()
