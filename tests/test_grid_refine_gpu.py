"""Grid refine (pof_grid_refine, N19) on the GPU: the device against the NumPy restatement of tests/test_grid_refine.py.
votes, count, iters_used, ok and moved are held exactly; correction, score, obs, pose and trans within TOL = 1e-10, the
tolerance the ICP tests use against their restatement (tests/test_scan_match_gpu.py) -- the restatement adds in the
device's order, so what is left is the last bit of the one sincos per evaluation -- and BIT FOR BIT where no sincos
result enters: s0 and count of every scene whose incoming heading is 0 (sincos(0) is exact), and every output of a fit
that stops at its first evaluation there.  rot, which a moved pose is written with in float32, to one float32 ulp, and to
its incoming bits without ``moved``.  Every case's decisions are asserted to have been taken by a margin >= 1e-10 in
the restatement (tests/test_grid_refine.py does that for the committed cases without a GPU; the cases formed here from
device results assert it themselves).  The grids are built on the CPU by ``grid_map_oracle`` and uploaded."""
import os
import sys

import numpy as np
import pytest
import torch

from test_grid_map import grid_map_oracle
from test_grid_match import CELL, drive, pose_terms
from test_grid_refine import (DEFAULTS, EXACT, MARGIN_MIN, OUT_DTYPES, OUT_FIELDS, TOL, device_cases,
                              grid_refine_oracle, room_case, rule_cases, run_case, smallest_margins)

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "planar_optical_flow_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

CLOSE = ("correction", "score", "obs", "pose", "trans")


@pytest.fixture(scope="module")
def ops():
    from planar_optical_flow_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def cases():
    return device_cases()


def _cuda(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def _terms(sensor):
    """The incoming pose terms of a sensor: its own, or those of its pose."""
    rot, trans = pose_terms(sensor["pose"])
    return np.asarray(sensor.get("rot", rot), np.float32).reshape(4), np.asarray(sensor.get("trans", trans), np.float64)


def _inputs(ops, case, sensors):
    """-> (ranges, tab, rot, trans, pose, state) on the device and the NMS keywords."""
    stack = lambda k, dt: _cuda(np.stack([np.asarray(s[k]) for s in sensors]), dt)
    nms = {}
    if "inst" in sensors[0]:
        nms = dict(instance_mask=stack("inst", np.int32), num_det=stack("num_det", np.int32),
                   det_cls=stack("det_cls", np.float64))
    state = ops.GridMapState(stack("grid", np.int16), stack("origin", np.float64))
    rot = _cuda(np.stack([_terms(s)[0] for s in sensors]), np.float32)
    trans = _cuda(np.stack([_terms(s)[1] for s in sensors]), np.float64)
    return (stack("ranges", np.float32), _cuda(case["tab"], np.float64), rot, trans, stack("pose", np.float64), state), nms


def _host(out, rot, trans, pose):
    got = {k: getattr(out, k).cpu().numpy() for k in OUT_FIELDS}
    got.update(rot=rot.cpu().numpy().reshape(-1, 4), trans=trans.cpu().numpy(), pose=pose.cpu().numpy())
    return got


def dev_case(ops, case, sensors=None):
    """The device's outputs and pose terms for the sensors of a case in one batch, on the host."""
    sensors = case["sensors"] if sensors is None else sensors
    args, nms = _inputs(ops, case, sensors)
    grid = args[5].grid.clone()
    out = ops.grid_refine(*args, res=case["res"], **nms, **case["kw"])
    assert torch.equal(grid, args[5].grid)                     # the grid is read only
    return _host(out, args[2], args[3], args[4])


def assert_matches(got, b, want, sensor, what):
    """Sensor b of the device's results against the restatement's dict."""
    for k, dt in zip(OUT_FIELDS, OUT_DTYPES):
        assert got[k].dtype == dt, k
    for k in EXACT:
        assert np.array_equal(got[k][b], want[k]), (what, b, k, got[k][b], want[k])
    for k in CLOSE:
        x, y = np.asarray(got[k][b], np.float64), np.asarray(want[k], np.float64)
        assert np.array_equal(np.isnan(x), np.isnan(y)), (what, b, k, x, y)
        fin = ~np.isnan(y)
        assert np.abs(x[fin] - y[fin]).max(initial=0.0) <= TOL, (what, b, k, x, y)
    rot_in, trans_in = _terms(sensor)
    if want["moved"]:
        assert np.all(np.abs(got["rot"][b] - want["rot"]) <= np.spacing(np.abs(want["rot"]))), (what, b)   # one float32 ulp
        assert got["trans"][b].tobytes() == got["pose"][b, :2].tobytes()
        assert np.array_equal(got["pose"][b], np.asarray(sensor["pose"], np.float64) + got["correction"][b]), (what, b)
    else:                                                      # nothing is stored: the incoming bits
        assert got["rot"][b].tobytes() == rot_in.tobytes() and got["trans"][b].tobytes() == trans_in.tobytes(), (what, b)
        assert got["pose"][b].tobytes() == np.asarray(sensor["pose"], np.float64).tobytes(), (what, b)
        assert not got["correction"][b].any()
    if float(sensor["pose"][2]) == 0.0:                        # no sincos result enters the first evaluation
        assert got["score"][b, :1].tobytes() == np.asarray(want["score"][:1]).tobytes(), (what, b, "s0")
        if int(want["iters_used"]) == 0:
            for k in CLOSE:
                assert got[k][b].tobytes() == np.asarray(want[k], np.float64).tobytes(), (what, b, k)


def check_case(ops, case, what, margins=True):
    got, want = dev_case(ops, case), run_case(case)
    if margins:
        small = smallest_margins(want)
        assert all(v >= MARGIN_MIN for v in small.values()), (what, small)
    for b, (s, w) in enumerate(zip(case["sensors"], want)):
        assert_matches(got, b, w, s, what)
    return got, want


# ------------------------------------------------------------------ 1. the device against the restatement
# The rule scenes of tests/test_grid_refine.rule_cases.  Its gate_cases stand at equality on purpose and stay on the CPU:
# a decision nearer to equality than TOL is the restatement's to take.  At phi = 0 a painted wall puts points on a cell
# border and "not better" has s1 = s0: there the decisions hold by exact arithmetic (sincos(0) is exact), not by a margin.
def all_rule_cases():
    return rule_cases()


def embedded(case, N, at):
    """The scene of a rule case as the beams at, at + 1, ... of a scan of N beams without another return."""
    n = len(case["sensors"][0]["ranges"])
    tab = np.zeros(3 * N)
    tab[N + 2 * at:N + 2 * (at + n)] = case["tab"][n:]
    sensors = []
    for s in case["sensors"]:
        ranges = np.full(N, np.inf, np.float32)
        ranges[at:at + n] = s["ranges"]
        e = dict(s, ranges=ranges)
        if "inst" in s:
            inst, cls = np.zeros(N, np.int32), np.zeros(N)
            inst[at:at + n] = s["inst"]
            cls[:n] = s["det_cls"]
            e.update(inst=inst, det_cls=cls)
        sensors.append(e)
    return dict(case, tab=tab, sensors=sensors)


def _rule_margins_ok(name, want):
    small = smallest_margins(want)
    # the painted walls are symmetric tents with their points on the ridge: across that cell border the interpolant, A
    # and (with e = 0 there) b are continuous, so which side a point falls on decides nothing
    small.pop("cell", None)
    if name == "not better":                                   # s1 = s0 exactly
        return True
    return all(v >= MARGIN_MIN for v in small.values())


@pytest.mark.parametrize("name", sorted(all_rule_cases()))
def test_rule_scenes(ops, name):
    case = all_rule_cases()[name]
    got, want = check_case(ops, case, name, margins=False)
    assert _rule_margins_ok(name, want), name
    if name == "turned":
        return
    # at phi = 0 every sum is the restatement's sum: report whether the whole fit came out bit for bit
    same = all(got[k][0].tobytes() == np.asarray(want[0][k], np.float64).tobytes() for k in CLOSE)
    print("%s: iters_used %d, ok %d, moved %d, every float the restatement's bits: %s"
          % (name, got["iters_used"][0], got["ok"][0], got["moved"][0], same))


@pytest.mark.parametrize("N", [64, 65, 512, 513, 4096])
def test_rule_scenes_embedded_in_longer_scans(ops, N):
    """Start, middle and end of a scan of N beams: another thread, another slot, another wave own the points, and the
    restatement's sums follow them."""
    for name, case in sorted(all_rule_cases().items()):
        n = len(case["sensors"][0]["ranges"])
        for at in (0, (N - n) // 2 + 1, N - n):
            check_case(ops, embedded(case, N, at), (name, N, at), margins=False)


@pytest.mark.parametrize("name", sorted(device_cases()))
def test_shapes(ops, cases, name):
    got, want = check_case(ops, cases[name], name)
    print("%s: votes %s, count %s, iters_used %s, ok %s, moved %s" % (name, got["votes"].tolist(), got["count"].tolist(),
                                                                    got["iters_used"].tolist(), got["ok"].tolist(),
                                                                    got["moved"].tolist()))
    assert got["ok"].any()
    if name in ("64 x 128 with people", "N 512", "N 513", "N 4096"):
        assert got["moved"].any()


# ------------------------------------------------------------------ 2. determinism
def test_same_bits_at_five_batch_positions_and_in_two_runs(ops, cases):
    case = cases["64 x 128 with people"]
    me, other = case["sensors"][0], case["sensors"][2]
    want = run_case(dict(case, sensors=[me]))[0]
    runs = []
    for pos in list(range(5)) + [2]:
        sensors = [other] * 5
        sensors[pos] = me
        got = dev_case(ops, case, sensors)
        assert_matches(got, pos, want, me, pos)
        runs.append(got)
    for k in OUT_FIELDS + ("pose", "trans", "rot"):
        assert runs[2][k].tobytes() == runs[5][k].tobytes(), k                  # two runs: every sensor's bits
        for pos in range(1, 5):                                                 # one sensor at five positions
            assert runs[pos][k][pos].tobytes() == runs[0][k][0].tobytes(), (k, pos)


def test_a_captured_launch_replayed_over_six_inputs(ops, cases):
    case = cases["64 x 128 with people"]
    inputs = [dict(s, pose=s["pose"] + np.asarray(d)) for s in case["sensors"] for d in ((0.0, 0.0, 0.0), (0.015, 0.02, -0.003))]
    want = run_case(dict(case, sensors=inputs))
    small = smallest_margins(want)
    assert all(v >= MARGIN_MIN for v in small.values()), small
    (ranges, tab, rot, trans, pose, state), nms = _inputs(ops, case, inputs[:1])
    out = ops.grid_refine_buffers(1)
    call = lambda: ops.grid_refine(ranges, tab, rot, trans, pose, state, res=case["res"], out=out, **nms, **case["kw"])
    fresh = [(rot.clone(), trans.clone(), pose.clone())]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    moved = 0
    for s, w in zip(inputs, want):
        (r2, _, rot2, trans2, pose2, state2), nms2 = _inputs(ops, case, [s])
        for dst, src in ((ranges, r2), (rot, rot2), (trans, trans2), (pose, pose2), (state.grid, state2.grid),
                         (state.origin, state2.origin)) + tuple((nms[k], nms2[k]) for k in nms):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert_matches(_host(out, rot, trans, pose), 0, w, s, "replay")
        moved += int(w["moved"])
    assert moved >= 3 and fresh


# ------------------------------------------------------------------ 3. refused calls
def test_refused_calls_leave_outputs_and_pose_terms_untouched(ops):
    from planar_optical_flow_amd import _lib
    from planar_optical_flow_amd._lib import POF_E_BADARG, POF_E_SHAPE, PofError
    rng = np.random.default_rng(1)
    lib = _lib.load()
    ptr = lambda t: None if t is None else t.data_ptr()
    case = room_case(5, 64, 64, 64, people=True, min_points=5, max_range=6.0)

    def sentinel_call(N=64, H=64, drop=(), **kw):
        """The raw entry point on sentinel-filled outputs and pose terms -> (status, everything untouched)."""
        v = dict(dict(DEFAULTS, res=0.1), **kw)
        (ranges, tab, rot, trans, pose, state), nms = _inputs(ops, case, case["sensors"])
        if N > 64:
            ranges, tab = torch.ones(1, N, device="cuda"), torch.zeros(3 * N, dtype=torch.float64, device="cuda")
            nms = {k: torch.zeros((1, N), dtype=t.dtype, device="cuda") if t.dim() == 2 else t for k, t in nms.items()}
        grid = state.grid if H == 64 else torch.zeros(1, H, 64, dtype=torch.int16, device="cuda")
        out = ops.grid_refine_buffers(1)
        watched = (rot, trans, pose) + tuple(out)
        for t in watched:
            t.copy_(torch.from_numpy(rng.integers(1, 100, tuple(t.shape))).to(t.dtype))
        before = [t.cpu().numpy() for t in watched]
        gate = [None if k in drop else ptr(nms[k]) for k in ("instance_mask", "num_det", "det_cls")]
        rc = lib.pof_grid_refine(ptr(ranges), ptr(tab), *gate, v["cls_thresh"], v["max_range"], ptr(grid),
                                 ptr(state.origin), v["res"], v["cap"], v["iters"], v["min_points"], v["min_pivot"],
                                 v["max_shift"], v["max_turn"], v["eps_shift"], v["eps_turn"], 1, N, H, 64, ptr(pose),
                                 ptr(rot), ptr(trans), *[ptr(t) for t in out], None)
        torch.cuda.synchronize()
        return rc, all(np.array_equal(a, t.cpu().numpy()) for a, t in zip(before, watched))

    assert sentinel_call(N=4097) == (POF_E_SHAPE, True)
    assert sentinel_call(H=96) == (POF_E_SHAPE, True)
    for kw in (dict(cap=0), dict(cap=32768), dict(iters=33), dict(iters=0), dict(res=0.0), dict(min_points=-1),
               dict(min_pivot=-1.0), dict(max_shift=float("nan")), dict(max_turn=-0.1), dict(max_range=0.0)):
        assert sentinel_call(**kw) == (POF_E_BADARG, True), kw
    for drop in (("num_det",), ("instance_mask",), ("num_det", "det_cls")):
        assert sentinel_call(drop=drop) == (POF_E_BADARG, True), drop
    # the wrapper: the same refusals as exceptions, and its own shape checks
    args, nms = _inputs(ops, case, case["sensors"])
    for kw, error in ((dict(cap=0), ValueError), (dict(iters=33), ValueError), (dict(max_turn=-1.0), ValueError),
                      (dict(res=0.0), AssertionError), (dict(max_range=0.0), AssertionError)):
        with pytest.raises(error):
            ops.grid_refine(*args, **dict(dict(res=0.1), **kw), **nms)
    with pytest.raises(PofError) as e:
        ops.grid_refine(torch.ones(1, 4097, device="cuda"), torch.zeros(3 * 4097, dtype=torch.float64, device="cuda"),
                        *args[2:], res=0.1)
    assert e.value.code == POF_E_SHAPE
    for part in (("instance_mask",), ("num_det", "det_cls"), ("instance_mask", "det_cls")):
        with pytest.raises(ValueError):
            ops.grid_refine(*args, res=0.1, **{k: nms[k] for k in part})
    with pytest.raises(ValueError):
        ops.grid_refine(*args, res=0.1, out=ops.grid_refine_buffers(2))
    with pytest.raises(ValueError):
        ops.grid_refine(*args[:4], torch.zeros(2, 3, dtype=torch.float64, device="cuda"), args[5], res=0.1)
    with pytest.raises(TypeError):
        ops.grid_refine(*args[:4], None, args[5], res=0.1)
    empty = ops.grid_refine(args[0][:0], args[1], args[2][:0], args[3][:0], args[4][:0], ops.grid_map_state(0, 64, 64), res=0.1)
    assert empty.correction.shape == (0, 3) and empty.ok.shape == (0,)
    # the next good call works
    check_case(ops, case, "after the refusals")


# ------------------------------------------------------------------ 4. the reference-shaped wrapper
def test_occupancy_grid_refine_equals_the_restatement(ops):
    import src.utils.utils as u
    tab_np, scans, truth = drive(21, spoil=False)
    N, res, size = 450, CELL, (128, 192)
    phi = tab_np[:N]
    og = u.OccupancyGrid(phi, res=res, size=size, max_range=10.0)
    for t in range(6):
        og.update(scans[t], truth[t])
    before = og.logodds.copy()
    tab = u._table_for(phi).cpu().numpy()
    moved = 0
    for off, kw in (((0.0, 0.0, 0.0), {}), ((0.03, -0.02, 0.005), {}), ((-0.04, 0.03, -0.004), dict(iters=3, cap=20))):
        odom = truth[6] + np.asarray(off)
        new, info = og.refine(scans[6], odom, **kw)
        want = grid_refine_oracle(scans[6], tab, odom, before, og.origin, res, **dict(DEFAULTS, max_range=10.0, **kw))
        assert all(v >= MARGIN_MIN for v in want["margins"].values()), want["margins"]
        for k in EXACT:
            assert info[k] == want[k], (k, info[k], want[k])
        for k in ("correction", "score", "obs"):
            assert np.abs(np.asarray(info[k]) - want[k]).max() <= TOL, k
        assert np.abs(new - want["pose"]).max() <= TOL and info["ok"]
        if info["moved"]:
            left = np.asarray(off) + info["correction"]
            assert np.hypot(*left[:2]) <= res / np.sqrt(2.0)
        moved += info["moved"]
    assert moved >= 2 and np.array_equal(og.logodds, before)   # refine does not update the grid
    with pytest.raises(ValueError):
        og.refine(scans[6], truth[6], res=0.2)
    with pytest.raises(ValueError):
        og.refine(scans[6], truth[6], reach=3)


# ------------------------------------------------------------------ 5. streaming detector
def _stream_model(seed):
    from planar_optical_flow_amd.src.depracted.model.dr_spaam import SpatialDROW
    torch.manual_seed(seed)
    return SpatialDROW(num_scans=5, num_pts=56, alpha=0.5, window_size=11, pedestrian_only=True).cuda().eval()


STREAM_T = 12


def _stream_scans(B):
    """[T,B,450]: ``drive``'s sensors, STREAM_T scans each."""
    return np.stack([drive(31 + b, spoil=False)[1][:STREAM_T] for b in range(B)], axis=1), drive(31, spoil=False)[0]


def _snapshot(det):
    """Everything the stage reads and leaves behind, on the host."""
    _, conf, num, inst = det._dets
    state, _ = det.grid_map()
    snap = {"det_cls": conf, "num_det": num, "inst": inst, "rot": det._pose_rot, "trans": det._pose_trans,
            "pose": det._pose_state, "grid": state.grid, "origin": state.origin}
    snap.update({k: getattr(det.grid_refine()[1], k) for k in OUT_FIELDS})
    return {k: v.detach().cpu().numpy().copy() for k, v in snap.items()}


@pytest.mark.parametrize("matched,scrolled", [(False, False), (True, False), (False, True), (True, True)])
def test_streaming_detector_eager_graph_and_restatement(matched, scrolled):
    from planar_optical_flow_amd.streaming import StreamingDetector
    B, size = 2, 192
    scans, tab_np = _stream_scans(B)
    model = _stream_model(13)
    kw = dict(batch=B, nms_min_dist=0.5, cls_thresh=0.5, ego_motion=dict(method="scan_match"), grid_map=dict(size=size),
              angle_inc=float(tab_np[1] - tab_np[0]))
    if matched:
        kw.update(grid_match=dict())
    if scrolled:
        kw.update(grid_scroll=dict(margin=64))
    eager = StreamingDetector(model, graph=False, grid_refine=dict(), **kw)
    graphed = StreamingDetector(model, graph=True, grid_refine=dict(), **kw)
    parent = StreamingDetector(model, graph=True, **kw)       # the detector as it was: no grid_refine
    assert parent._gr_kw is None and not hasattr(parent, "_gr_out") and len(graphed._stages) == len(parent._stages) + 1
    names = [s.launch.__name__ for s in graphed._stages]
    assert names == ["_match_stage"] + ["_grid_scroll_stage"] * scrolled + ["_grid_match_stage"] * matched + \
        ["_grid_refine_stage", "_grid_stage", "_keep_scan"]
    tab = graphed.tab.cpu().numpy()
    begin = (0.213, -0.127, 0.3)
    incoming = {}
    launch = eager._grid_refine_stage

    def recording(first):
        incoming.update(rot=eager._pose_rot.cpu().numpy().copy(), trans=eager._pose_trans.cpu().numpy().copy(),
                        pose=eager._pose_state.cpu().numpy().copy(), grid=eager._gm_state.grid.cpu().numpy().copy())
        launch(first)

    eager._stages = tuple(s._replace(launch=recording) if s.launch == launch else s for s in eager._stages)

    def run(check):
        for det in (eager, graphed):
            det.reset(pose=begin)
        fired, history = [], []
        for t in range(STREAM_T):
            for det in (eager, graphed):
                if t == 0:
                    with pytest.raises(RuntimeError):
                        det.grid_refine()
                det(torch.from_numpy(scans[t]).cuda())
            e, g = _snapshot(eager), _snapshot(graphed)
            for k in e:
                assert e[k].tobytes() == g[k].tobytes(), (t, k)    # eager and replayed: identical bits
            history.append(g)
            dicts, rec = graphed.grid_refine()
            assert rec is graphed._gr_out and len(dicts) == B
            for b in range(B):
                assert dicts[b]["moved"] == bool(g["moved"][b]) and dicts[b]["votes"] == int(g["votes"][b])
                assert np.array_equal(dicts[b]["correction"], g["correction"][b])
            fired.append(g["moved"].astype(bool).tolist())
            if not check:
                continue
            for b in range(B):                                     # the step against the restated chain
                want = grid_refine_oracle(scans[t, b], tab, incoming["pose"][b], incoming["grid"][b], e["origin"][b],
                                          0.1, e["inst"][b], e["num_det"][b], e["det_cls"][b], rot=incoming["rot"][b],
                                          trans=incoming["trans"][b], **DEFAULTS)
                assert all(v >= MARGIN_MIN for v in want["margins"].values()), (t, b, want["margins"])
                got = {k: e[k] for k in OUT_FIELDS + ("pose", "trans")}
                got["rot"] = e["rot"].reshape(B, 4)
                assert_matches(got, b, want, dict(pose=incoming["pose"][b], rot=incoming["rot"][b],
                                                  trans=incoming["trans"][b]), (t, b))
                grid = incoming["grid"][b].copy()                  # the scan went into the map at the refined pose
                grid_map_oracle(scans[t, b], tab, e["rot"][b], e["trans"][b], grid, e["origin"][b], 0.1, e["inst"][b],
                                e["num_det"][b], e["det_cls"][b])
                assert np.array_equal(grid, e["grid"][b]), (t, b)
        return fired, history

    fired, history = run(True)
    print("matched=%s scrolled=%s: moved per scan %s" % (matched, scrolled, fired))
    assert not any(fired[0]) and sum(any(f) for f in fired) >= STREAM_T // 2      # an empty grid moves nothing
    assert graphed._graph is not None and eager._graph is None
    again_fired, again = run(False)                            # reset() in between: the same bits once more
    assert again_fired == fired
    for a, b in zip(history, again):
        assert all(a[k].tobytes() == b[k].tobytes() for k in a)


def test_streaming_detector_constructor_rules():
    from planar_optical_flow_amd.streaming import StreamingDetector
    model = _stream_model(13)

    class DiffFlow(torch.nn.Module):
        def forward(self, prev, cur):
            return torch.cat([cur - prev, prev - cur], dim=2)

    match = dict(method="scan_match")
    for bad in (dict(grid_map=dict(size=64)),                                             # a pose per call
                dict(ego_motion=match),                                                   # no grid to fit to
                dict(ego_motion=dict(method="keyframe"), grid_map=dict(size=64)),
                dict(ego_motion=dict(method="keyframe_map"), grid_map=dict(size=64)),
                dict(ego_motion=match, grid_map=dict(size=64), nms_min_dist=0.5, flow_model=DiffFlow()),
                dict(ego_motion=dict(), grid_map=dict(size=64), nms_min_dist=0.5, flow_model=DiffFlow())):
        with pytest.raises(ValueError):
            StreamingDetector(model, grid_refine=dict(), **bad)
    for bad in (dict(cap=0), dict(iters=33), dict(min_points=-1), dict(max_shift=-1.0), dict(cls_thresh=0.5),
                dict(res=0.1), dict(reach=4)):
        with pytest.raises(ValueError):
            StreamingDetector(model, ego_motion=match, grid_map=dict(size=64), grid_refine=bad)
    plain = StreamingDetector(model, ego_motion=match, grid_map=dict(size=64))
    assert plain._gr_kw is None and not any(name.startswith("_gr_") and name != "_gr_kw" for name in dir(plain))
    with pytest.raises(RuntimeError):
        plain.grid_refine()
    det = StreamingDetector(model, ego_motion=match, grid_map=dict(size=(64, 128), res=0.125),
                            grid_refine=dict(iters=4, min_points=10))
    assert det._gr_out.correction.shape == (1, 3) and det._gr_kw["min_points"] == 10 and det._gr_kw["iters"] == 4
    assert [s.launch.__name__ for s in det._stages] == ["_match_stage", "_grid_refine_stage", "_grid_stage", "_keep_scan"]
    det(torch.zeros(450).cuda() + 3.0)
    dicts, rec = det.grid_refine()
    assert rec is det._gr_out and dicts[0]["ok"] is False and dicts[0]["moved"] is False     # an empty grid: A = 0
    assert dicts[0]["votes"] == 450 and dicts[0]["iters_used"] == 0 and not rec.correction.any()
