"""Keyframe scan matching (pof_keyframe_match, N9) on the GPU: short sequences with the state carried on the device
from step to step against the NumPy restatement of tests/test_keyframe.py -- exact in everything discrete and in the
stored keyframe, inside the tolerance derived there in the rest -- at the sizes where the launch changes form, at its
limits, in a captured graph and as the pose of the streaming detector."""
import ctypes

import numpy as np
import pytest
import torch

from test_keyframe import (SETTINGS, SEEDS, SHAPES, T_GPU, VARIANTS, assert_step_matches, rotating_case, scenario,
                           sequence_tolerance, shape_case)

pytestmark = pytest.mark.gpu

OUT = ("motion", "count", "rms", "ok", "iters_used", "obs", "key_replaced", "corr", "flow_residual")
STATE = ("key_ranges", "key_pose", "key_rel", "key_valid", "key_age", "key_misses", "pose")
TERMS = ("rot", "trans", "flow_trans")


@pytest.fixture(scope="module")
def ops():
    from planar_optical_flow_amd import ops as _ops
    return _ops


def _cuda(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


class Device:
    """B sensors on the device: the state, the outputs and the pose terms in fixed buffers; step(t) runs one launch
    and returns host copies of everything, one dict per field."""

    def __init__(self, ops, tab, scans, pose0, gates, kw):
        self.ops, self.tab, self.kw = ops, tab, kw
        T, B, N = scans.shape
        self.scans = _cuda(scans, np.float32)
        self.gates = None if gates is None else [
            dict(instance_mask=_cuda(np.stack([g[0][t] for g in gates]), np.int32),
                 num_det=_cuda(np.array([g[1][t] for g in gates]), np.int32),
                 det_cls=_cuda(np.stack([g[2][t] for g in gates]), np.float64)) for t in range(T)]
        self.state = ops.keyframe_buffers(B, N)
        self.out = ops.keyframe_match_buffers(B, N)
        self.terms = dict(rot=torch.zeros(B, 4, device="cuda"), trans=torch.zeros(B, 2, dtype=torch.float64, device="cuda"),
                          flow_trans=torch.zeros(B, 2, dtype=torch.float64, device="cuda"))
        self.pose0 = _cuda(pose0, np.float64)
        self.reset()

    def reset(self):
        self.ops.keyframe_reset(self.state, self.pose0)

    def launch(self, t):
        self.ops.keyframe_match(self.scans[t], self.tab, self.state, out=self.out, **({} if self.gates is None else self.gates[t]),
                                **self.terms, **self.kw)

    def host(self):
        got = {k: getattr(self.out, k).cpu().numpy() for k in OUT}
        got.update({k: getattr(self.state, k).cpu().numpy() for k in STATE})
        got.update({k: v.cpu().numpy() for k, v in self.terms.items()})
        return got

    def step(self, t):
        self.launch(t)
        return self.host()


def _sensor(host, b):
    return {k: v[b] for k, v in host.items()}


def _same_bits(a, b, what=""):
    for k in OUT + STATE + TERMS:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _oracle(tab_host, scans, poses, gates, kw):
    return sequence_tolerance([((scans[:, b], tab_host, poses[0, b]), dict(kw, persons=None if gates is None else gates[b][3]))
                               for b in range(scans.shape[1])])


# ------------------------------------------------------------------ 1. device against the restatement, every form
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("N", sorted(SHAPES))
def test_device_matches_the_restatement_over_a_sequence(ops, N, variant):
    inc, scans, poses, gates, kw = shape_case(N, variant)
    tab = ops.phi_table(inc, N)
    tol, want = _oracle(tab.cpu().numpy(), scans, poses, gates, kw)
    dev = Device(ops, tab, scans, poses[0], gates, kw)
    B, replaced = scans.shape[1], 0
    for t in range(T_GPU):
        got = dev.step(t)
        for b in range(B):
            assert_step_matches(_sensor(got, b), _sensor(got, b), want[b][t], tol, (N, variant, t, b))
            assert got["ok"][b] == (t > 0)
        replaced += int(got["key_replaced"].sum()) if t else 0
        print("N=%d %s t=%d: replaced %s, age %s, matched %s, %s iterations"
              % (N, variant, t, got["key_replaced"], got["key_age"], got["count"], got["iters_used"]))
    err = np.hypot(*(got["pose"][:, :2] - poses[-1][:, :2]).T).max()
    print("N=%d %s: %d keyframes replaced after the seeding, final position error %.3e m" % (N, variant, replaced, err))
    assert all(sum(int(o["key_replaced"]) for _, o in want[b][1:]) >= 1 for b in range(B))


# ------------------------------------------------------------------ 2. limits: error codes, nothing written
def _raw(ops, cur, tab, state, out, window=16, N=None, B=None):
    from planar_optical_flow_amd import _lib
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    return _lib.load().pof_keyframe_match(p(cur), p(tab), None, None, None, 0.5, 20.0, window, 0.5, 0.3, 0.05, 16, 1e-7,
                                          1e-7, 1e-6, 0.3, 0.3, 0.5, 2, cur.shape[0] if B is None else B,
                                          cur.shape[1] if N is None else N, *[p(t) for t in state], *[p(t) for t in out],
                                          None, None, None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_limits_return_their_codes_and_leave_state_and_outputs_alone(ops):
    from planar_optical_flow_amd._lib import POF_E_BADARG, POF_E_SHAPE, POF_OK, PofError
    N = 4097
    tab = ops.phi_table(np.radians(0.05), N)
    r = torch.full((1, N), 5.0, device="cuda")
    state = ops.KeyframeState(*(torch.full_like(t, 7) for t in ops.keyframe_buffers(1, N)))
    out = ops.KeyframeMatch(*(torch.full_like(t, 7) for t in ops.keyframe_match_buffers(1, N)))
    assert _raw(ops, r, tab, state, out) == POF_E_SHAPE
    assert _raw(ops, r, tab, state, out, window=65, N=4096) == POF_E_BADARG
    assert _raw(ops, r, tab, state, out, B=0, N=4096) == POF_OK
    with pytest.raises(PofError) as e:
        ops.keyframe_match(r, tab, state, out=out)
    assert e.value.code == POF_E_SHAPE
    torch.cuda.synchronize()
    for t in tuple(state) + tuple(out):
        assert (t == 7).all()
    empty_state = ops.keyframe_buffers(0, 70)
    empty = ops.keyframe_match(torch.zeros(0, 70, device="cuda"), ops.phi_table(np.radians(0.5), 70), empty_state)
    assert empty.motion.shape == (0, 3) and empty.corr.shape == (0, 70) and empty.key_replaced.shape == (0,)
    with pytest.raises(ValueError):
        ops.keyframe_match(r[:, :70].contiguous(), ops.phi_table(np.radians(0.5), 70), ops.keyframe_buffers(1, 71))
    with pytest.raises(ValueError):
        ops.keyframe_match(r[:, :70].contiguous(), ops.phi_table(np.radians(0.5), 70), ops.keyframe_buffers(1, 70),
                           out=ops.keyframe_match_buffers(1, 71))


# ------------------------------------------------------------------ 3. determinism
@pytest.mark.parametrize("N", [450, 513])
def test_the_same_bits_at_every_batch_position_in_every_run_and_in_a_graph(ops, N):
    inc, scans, poses, gates, kw = shape_case(N, "gated")
    tab = ops.phi_table(inc, N)
    five = lambda a: np.repeat(a[:, :1], 5, axis=1)
    dev = Device(ops, tab, five(scans), five(poses)[0], [gates[0]] * 5, kw)
    first = [dev.step(t) for t in range(T_GPU)]
    dev.reset()
    second = [dev.step(t) for t in range(T_GPU)]
    single = Device(ops, tab, scans[:, :1], poses[0, :1], gates[:1], kw)
    for t in range(T_GPU):
        _same_bits(first[t], second[t], t)
        for b in range(1, 5):
            _same_bits(_sensor(first[t], 0), _sensor(first[t], b), (t, b))
        _same_bits(_sensor(first[t], 0), _sensor(single.step(t), 0), t)
    assert sum(int(f["key_replaced"][0]) for f in first[1:]) >= 1 and all(f["ok"].all() for f in first[1:])
    # one step captured on fixed input buffers, replayed over the sequence twice with the state restored in between
    cur = torch.zeros_like(dev.scans[0])
    gate = {k: torch.zeros_like(v) for k, v in dev.gates[0].items()}
    call = lambda: ops.keyframe_match(cur, tab, dev.state, out=dev.out, **gate, **dev.terms, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                  # warm-up; the state it moved is restored below
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for _ in range(2):
        dev.reset()
        for t in range(T_GPU):
            cur.copy_(dev.scans[t])
            for k in gate:
                gate[k].copy_(dev.gates[t][k])
            graph.replay()
            _same_bits(dev.host(), first[t], t)


# ------------------------------------------------------------------ 4. outside the keyframe's field of view
def test_points_that_project_outside_the_keyframes_field_of_view(ops):
    scans, poses, kw = rotating_case()
    tab = ops.phi_table()
    tol, (want,) = sequence_tolerance([((scans, tab.cpu().numpy(), poses[0]), kw)])
    dev = Device(ops, tab, scans[:, None], poses[:1], None, kw)
    for t in range(len(scans)):
        got = _sensor(dev.step(t), 0)
        assert_step_matches(got, got, want[t], tol, t)
    outside = int(round(0.5 / np.radians(0.5))) - 16
    assert got["ok"] and (got["corr"][450 - outside:] == -1).all() and got["corr"].max() == 449 and got["key_age"] == 5


# ------------------------------------------------------------------ 5. utils
def test_utils_keyframe_odometry_numpy_in_numpy_out(ops):
    import os
    import sys
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "planar_optical_flow_amd")
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    import src.utils.utils as u
    from oracle import ref_numpy as R
    inc, scans, poses, _, kw = shape_case(450, "huber")
    dev = Device(ops, ops.phi_table(), scans[:, :1], poses[0, :1], None, kw)
    odo = u.KeyframeOdometry(R.laser_phi(), **kw)
    odo.reset(poses[0, 0])
    for t in range(4):
        res, want = odo.update(scans[t, 0]), _sensor(dev.step(t), 0)
        for k in ("pose", "motion", "count", "rms", "iters_used", "obs", "key_age", "key_misses", "key_pose", "corr",
                  "flow_residual"):
            assert np.array_equal(np.asarray(res[k]), want[k], equal_nan=True), (t, k)
        assert isinstance(res["ok"], bool) and res["ok"] == (t > 0) and res["key_replaced"] == bool(want["key_replaced"])
    with pytest.raises(ValueError):
        u.KeyframeOdometry(R.laser_phi(), delta=1.0)
    # with predictions the NMS runs first: confident detections everywhere leave nothing to become a keyframe
    odo.reset()
    res = odo.update(scans[0, 0], pred_cls=np.full((450, 1), 0.9), pred_reg=np.zeros((450, 2)))
    assert not res["ok"] and res["key_replaced"] and np.array_equal(res["pose"], np.zeros(3))
    gated = np.isnan(odo._state.key_ranges.cpu().numpy()).sum()
    odo.reset()
    odo.update(scans[0, 0], pred_cls=np.full((450, 1), 0.1), pred_reg=np.zeros((450, 2)))
    assert gated > np.isnan(odo._state.key_ranges.cpu().numpy()).sum()     # low scores gate nothing


# ------------------------------------------------------------------ 6. streaming detector
def _stream_model(seed):
    from planar_optical_flow_amd.src.depracted.model.dr_spaam import SpatialDROW
    torch.manual_seed(seed)
    return SpatialDROW(num_scans=5, num_pts=56, alpha=0.5, window_size=11, pedestrian_only=True).cuda().eval()


class _BufferFlow(torch.nn.Module):
    """A 'flow net' that returns a registered buffer: (previous scan, scan) [B,N,1] -> [B,N,2]."""

    def __init__(self, B, N):
        super().__init__()
        self.register_buffer("flow", torch.zeros(B, N, 2))

    def forward(self, prev, cur):
        return self.flow


@pytest.mark.parametrize("name", ["still", "walk"])
def test_streaming_detector_keeps_its_pose_from_the_scans_alone(ops, name):
    from planar_optical_flow_amd.streaming import StreamingDetector
    B, T = 2, 9
    seqs = [scenario(name, SEEDS[b]) for b in range(B)]
    scans, poses = np.stack([s[0][:T] for s in seqs], axis=1), np.stack([s[1][:T] for s in seqs], axis=1)
    model = _stream_model(13)
    mk = lambda graph: StreamingDetector(model, batch=B, graph=graph, ego_motion=dict(method="keyframe"))
    eager, graphed = mk(False), mk(True)
    assert eager._flow_model is None and eager._nms is None and eager._match_kw is None and not hasattr(eager, "_match_out")
    for det in (eager, graphed):
        with pytest.raises(RuntimeError):
            det.ego_motion()
        det.reset(pose=poses[0])
    with pytest.raises(ValueError):
        graphed(scans[0], pose=poses[0])
    tol, want = sequence_tolerance([((scans[:, b], graphed.tab.cpu().numpy(), poses[0, b]), SETTINGS) for b in range(B)])
    dev = torch.from_numpy(scans).cuda()
    for t in range(T):
        eager(dev[t]), graphed(dev[t])
        (me, oe), (mg, og) = eager.ego_motion(), graphed.ego_motion()
        for k in OUT:
            assert np.array_equal(getattr(oe, k).cpu().numpy(), getattr(og, k).cpu().numpy(), equal_nan=True), (t, k)
        for a, b_ in zip(eager._key_state, graphed._key_state):
            assert torch.equal(a.view(torch.uint8), b_.view(torch.uint8)), t
        host = {k: getattr(og, k).cpu().numpy() for k in OUT}
        host.update({k: getattr(graphed._key_state, k).cpu().numpy() for k in STATE})
        for b in range(B):
            assert_step_matches(_sensor(host, b), _sensor(host, b), want[b][t], tol, (name, t, b))
            assert set(mg[b]) == {"motion", "ok", "count", "rms", "iters_used", "obs", "pose", "key_replaced", "key_age",
                                  "key_pose"}
            assert mg[b]["ok"] == (t > 0) and mg[b]["key_age"] == int(want[b][t][0]["key_age"])
            assert np.array_equal(mg[b]["pose"], host["pose"][b]) and np.array_equal(mg[b]["key_pose"], host["key_pose"][b])
    assert graphed._graph is not None and eager._graph is None
    err = np.hypot(*(host["pose"][:, :2] - poses[-1][:, :2]).T).max()
    print("%s: position error after %d scans %.3e m, keyframe ages %s" % (name, T, err, host["key_age"]))
    if name == "still":
        assert (host["key_age"] == T - 1).all()
    # a new sequence from a pose of the caller's: the first scan seeds again
    graphed.reset(pose=[1.0, 2.0, 0.3])
    graphed(dev[0])
    fit, _ = graphed.ego_motion()
    for b in range(B):
        assert not fit[b]["ok"] and fit[b]["key_replaced"] and fit[b]["key_age"] == 0
        assert np.array_equal(fit[b]["pose"], [1.0, 2.0, 0.3]) and np.array_equal(fit[b]["key_pose"], [1.0, 2.0, 0.3])


def test_streaming_settings_and_what_the_other_methods_allocate():
    from planar_optical_flow_amd.streaming import StreamingDetector
    B = 2
    model, stub = _stream_model(13), _BufferFlow(B, 450).cuda()
    for kw in (dict(), dict(nms_min_dist=0.5, flow_model=stub), dict(ego_motion=dict(method="scan_match")),
               dict(nms_min_dist=0.5, flow_model=stub, ego_motion=dict(method="flow"))):
        other = StreamingDetector(model, batch=B, **kw)
        assert other._key_kw is None and not hasattr(other, "_key_state") and not hasattr(other, "_key_out"), kw
    for bad in (dict(method="keyframe", delta=1.0), dict(method="keyframes")):
        with pytest.raises(ValueError):
            StreamingDetector(model, batch=B, ego_motion=bad)
    with pytest.raises(ValueError):
        StreamingDetector(model, batch=B, ego_motion=dict(method="keyframe"), tracks=dict())    # tracks need the flow
    det = StreamingDetector(model, batch=B, ego_motion=dict(method="keyframe", key_dist=0.1, max_misses=0))
    assert det._key_kw["key_dist"] == 0.1 and det._key_kw["max_misses"] == 0 and det._key_kw["key_rot"] == 0.3
    assert det._pose_state.data_ptr() == det._key_state.pose.data_ptr()


def test_streaming_detector_with_a_flow_model_reads_the_pose_terms_this_launch_wrote(ops):
    from planar_optical_flow_amd.streaming import StreamingDetector
    from test_scan_match import person_points
    B, T = 1, 5
    scans, poses, _ = scenario("walk", SEEDS[2])
    model, stub = _stream_model(13), _BufferFlow(B, 450).cuda()
    stub.flow.normal_(0, 0.02)
    cfg = dict(method="keyframe", cls_thresh=0.5, key_dist=0.02)    # every step of this walk is longer: 0.033 m and up
    mk = lambda graph: StreamingDetector(model, batch=B, graph=graph, nms_min_dist=0.5, flow_model=stub, ego_motion=cfg)
    eager, graphed = mk(False), mk(True)
    assert not hasattr(graphed, "_ego_out") and not hasattr(graphed, "_match_out")
    eager.reset(pose=poses[0]), graphed.reset(pose=poses[0])
    dev = torch.from_numpy(scans[:T, None]).cuda()
    replaced = 0
    for t in range(T):
        eager(dev[t]), graphed(dev[t])
        (me, oe), (mg, og) = eager.ego_motion(), graphed.ego_motion()
        for k in OUT:
            assert np.array_equal(getattr(oe, k).cpu().numpy(), getattr(og, k).cpu().numpy(), equal_nan=True), (t, k)
        replaced += int(mg[0]["key_replaced"]) if t else 0
        # the pose terms are the pose's: the launch wrote them itself
        pose = mg[0]["pose"]
        assert np.array_equal(graphed._pose_trans[0].cpu().numpy(), pose[:2])
        c, s = np.cos(pose[2]), np.sin(pose[2])
        np.testing.assert_allclose(graphed._pose_rot[0].cpu().numpy().reshape(-1), [c, -s, s, c], rtol=0, atol=1e-7)
        # the gate: the points of this scan's confident detections have no correspondence and are no vertices
        dets, inst = graphed.detections()
        person = person_points(inst[0], len(dets[0][1]), np.concatenate([dets[0][1], np.zeros(450 - len(dets[0][1]))]))
        assert (og.corr[0].cpu().numpy()[person] == -1).all()
        if mg[0]["key_replaced"]:
            assert np.isnan(graphed._key_state.key_ranges[0].cpu().numpy()[person]).all()
        if t == 0:
            for det in (eager, graphed):
                with pytest.raises(RuntimeError):
                    det.person_flow()
            last_pose = pose.copy()
            continue
        (pe, fe), (pg, fg) = eager.person_flow(), graphed.person_flow()
        for k in fe._fields:
            assert np.array_equal(getattr(fe, k).cpu().numpy(), getattr(fg, k).cpu().numpy(), equal_nan=True), (t, k)
        xy, conf, num, inst_dev = graphed._dets
        ref = ops.person_flow(stub.flow.float().contiguous(), graphed.tab, inst_dev, num, xy, conf, graphed._pose_rot,
                              graphed._pose_trans, graphed._pose_flow_trans, 0.5)
        for k in ref._fields:
            assert np.array_equal(getattr(ref, k).cpu().numpy(), getattr(fg, k).cpu().numpy(), equal_nan=True), (t, k)
        if mg[0]["ok"]:
            assert np.array_equal(graphed._pose_flow_trans[0].cpu().numpy(), pose[:2] - last_pose[:2])
        last_pose = pose.copy()
    assert replaced >= 1
