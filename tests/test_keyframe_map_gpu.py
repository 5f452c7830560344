"""The keyframe map (pof_keyframe_map_match, N10) on the GPU: ten scans of an out-and-back walk with the state carried
on the device against the NumPy restatement of tests/test_keyframe_map.py -- exact in everything discrete and in every
stored keyframe row, inside the tolerance derived there in the rest -- at the sizes where the launch changes form, with
one slot against pof_keyframe_match, at its limits, in a captured graph and as the pose of the streaming detector."""
import ctypes

import numpy as np
import pytest
import torch

from test_keyframe import SETTINGS
from test_keyframe_gpu import _BufferFlow, _cuda, _sensor, _stream_model
from test_keyframe_map import (KEY_DIST_GPU, KEYS_GPU, MAP, SHAPES, T_GPU, VARIANTS, assert_fills_evicts_and_switches,
                               assert_map_step_matches, case_oracle, map_tolerance, shape_case, stream_case)

pytestmark = pytest.mark.gpu

OUT = ("motion", "count", "rms", "ok", "iters_used", "obs", "key_replaced", "key_switched", "key_slot", "corr",
       "flow_residual")
STATE = ("key_ranges", "key_pose", "key_valid", "key_stamp", "key_active", "key_rel", "key_age", "key_misses", "step",
         "pose")
TERMS = ("rot", "trans", "flow_trans")


@pytest.fixture(scope="module")
def ops():
    from planar_optical_flow_amd import ops as _ops
    return _ops


class Device:
    """B sensors on the device: the ring, the outputs and the pose terms in fixed buffers; step(t) runs one launch
    and returns host copies of everything, one dict per field."""

    def __init__(self, ops, tab, scans, pose0, gates, kw, keys):
        self.ops, self.tab, self.kw = ops, tab, kw
        T, B, N = scans.shape
        self.scans = _cuda(scans, np.float32)
        self.gates = None if gates is None else [
            dict(instance_mask=_cuda(np.stack([g[0][t] for g in gates]), np.int32),
                 num_det=_cuda(np.array([g[1][t] for g in gates]), np.int32),
                 det_cls=_cuda(np.stack([g[2][t] for g in gates]), np.float64)) for t in range(T)]
        self.state = ops.keyframe_map_buffers(B, N, keys)
        self.out = ops.keyframe_map_match_buffers(B, N)
        self.terms = dict(rot=torch.zeros(B, 4, device="cuda"), trans=torch.zeros(B, 2, dtype=torch.float64, device="cuda"),
                          flow_trans=torch.zeros(B, 2, dtype=torch.float64, device="cuda"))
        self.pose0 = _cuda(pose0, np.float64)
        self.reset()

    def reset(self):
        self.ops.keyframe_map_reset(self.state, self.pose0)

    def launch(self, t):
        self.ops.keyframe_map_match(self.scans[t], self.tab, self.state, out=self.out,
                                    **({} if self.gates is None else self.gates[t]), **self.terms, **self.kw)

    def host(self):
        got = {k: getattr(self.out, k).cpu().numpy() for k in OUT}
        got.update({k: getattr(self.state, k).cpu().numpy() for k in STATE})
        got.update({k: v.cpu().numpy() for k, v in self.terms.items()})
        return got

    def step(self, t):
        self.launch(t)
        return self.host()


def _same_bits(a, b, what=""):
    for k in OUT + STATE + TERMS:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _against_the_restatement(ops, case, what):
    inc, scans, poses, gates, kw, keys = case
    tab = ops.phi_table(inc, scans.shape[2])
    tol, want = case_oracle(case)
    dev = Device(ops, tab, scans, poses[0], gates, kw, keys)
    for t in range(scans.shape[0]):
        got = dev.step(t)
        for b in range(scans.shape[1]):
            assert_map_step_matches(_sensor(got, b), want[b][t], tol, what + (t, b))
        print("%s t=%d: slot %s, stored %s, switched %s, age %s, matched %s, %s iterations"
              % (what, t, got["key_slot"], got["key_replaced"], got["key_switched"], got["key_age"], got["count"],
                 got["iters_used"]))
    return got, want


# ------------------------------------------------------------------ 1. device against the restatement, every form
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("N", sorted(SHAPES))
def test_device_matches_the_restatement_over_a_return(ops, N, variant):
    got, want = _against_the_restatement(ops, shape_case(N, variant), (N, variant))
    for steps in want:
        assert_fills_evicts_and_switches(steps)                # the ring fills, slot 0 is evicted, one switch
    assert (got["key_valid"] == 1).all() and (got["key_slot"] == 2).all() and (got["step"] == T_GPU).all()


def test_device_matches_the_restatement_with_sixty_four_slots(ops):
    got, want = _against_the_restatement(ops, shape_case(450, "huber", keys=64), (450, "K=64"))
    assert got["key_ranges"].shape == (3, 64, 450) and (got["key_valid"].sum(axis=1) == 4).all()
    assert (got["key_slot"] == 2).all() and not got["key_ranges"][:, 4:].any() and not got["key_pose"][:, 4:].any()


# ------------------------------------------------------------------ 2. one slot is pof_keyframe_match
@pytest.mark.parametrize("N", [450, 513])
def test_one_slot_has_the_bits_of_keyframe_match(ops, N):
    inc, scans, poses, gates, kw, _ = shape_case(N, "gated")
    tab = ops.phi_table(inc, N)
    B = scans.shape[1]
    ring = Device(ops, tab, scans, poses[0], gates, kw, 1)
    single, single_out = ops.keyframe_buffers(B, N), ops.keyframe_match_buffers(B, N)
    terms = {k: torch.zeros_like(v) for k, v in ring.terms.items()}
    ops.keyframe_reset(single, ring.pose0)
    n9 = {k: v for k, v in kw.items() if k != "revisit"}
    replaced = 0
    for t in range(T_GPU):
        got = ring.step(t)
        ops.keyframe_match(ring.scans[t], tab, single, out=single_out, **ring.gates[t], **terms, **n9)
        for k in single_out._fields:
            assert np.array_equal(got[k], getattr(single_out, k).cpu().numpy(), equal_nan=True), (t, k)
        for k in single._fields:
            assert np.array_equal(got[k].reshape(getattr(single, k).shape), getattr(single, k).cpu().numpy(),
                                  equal_nan=True), (t, k)
        for k in TERMS:
            assert np.array_equal(got[k], terms[k].cpu().numpy()), (t, k)
        assert not got["key_switched"].any() and not got["key_slot"].any() and (got["key_stamp"] == t).all()
        replaced += int(got["key_replaced"].sum()) if t else 0
    assert replaced >= 3 * B


# ------------------------------------------------------------------ 3. limits: error codes, nothing written
def _raw(cur, tab, state, out, N=None, keys=None, revisit=0.5):
    from planar_optical_flow_amd import _lib
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    return _lib.load().pof_keyframe_map_match(p(cur), p(tab), None, None, None, 0.5, 20.0, 16, 0.5, 0.3, 0.05, 16, 1e-7,
                                              1e-7, 1e-6, 0.3, 0.3, 0.5, 2, revisit, cur.shape[0],
                                              cur.shape[1] if N is None else N,
                                              state.key_ranges.shape[1] if keys is None else keys,
                                              *[p(t) for t in state], *[p(t) for t in out], None, None, None,
                                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_failure_statuses_leave_state_and_outputs_alone(ops):
    from planar_optical_flow_amd._lib import POF_E_BADARG, POF_E_SHAPE, PofError
    N = 4097
    tab = ops.phi_table(np.radians(0.05), N)
    r = torch.full((1, N), 5.0, device="cuda")
    state = ops.KeyframeMapState(*(torch.full_like(t, 7) for t in ops.keyframe_map_buffers(1, N, 2)))
    out = ops.KeyframeMapMatch(*(torch.full_like(t, 7) for t in ops.keyframe_map_match_buffers(1, N)))
    assert _raw(r, tab, state, out) == POF_E_SHAPE
    for keys in (0, 65):
        assert _raw(r, tab, state, out, N=4096, keys=keys) == POF_E_BADARG
    assert _raw(r, tab, state, out, N=4096, revisit=1.5) == POF_E_BADARG
    with pytest.raises(PofError) as e:
        ops.keyframe_map_match(r, tab, state, out=out)
    assert e.value.code == POF_E_SHAPE
    torch.cuda.synchronize()
    for t in tuple(state) + tuple(out):
        assert (t == 7).all()
    # the wrapper's own checks: shapes, dtypes, the ring size
    small, tab70 = r[:, :70].contiguous(), ops.phi_table(np.radians(0.5), 70)
    good = ops.keyframe_map_buffers(1, 70, 3)
    empty = ops.keyframe_map_match(torch.zeros(0, 70, device="cuda"), tab70, ops.keyframe_map_buffers(0, 70, 3))
    assert empty.motion.shape == (0, 3) and empty.key_switched.shape == (0,) and empty.key_slot.shape == (0,)
    z = lambda *shape, dtype=torch.int32: torch.zeros(*shape, dtype=dtype, device="cuda")
    for wrong in (ops.keyframe_map_buffers(1, 71, 3), ops.keyframe_map_buffers(2, 70, 3),
                  good._replace(key_ranges=z(1, 70, dtype=torch.float32)),
                  good._replace(key_ranges=z(1, 65, 70, dtype=torch.float32)),
                  good._replace(key_pose=z(1, 4, 3, dtype=torch.float64)), good._replace(key_stamp=z(1, 2)),
                  good._replace(key_active=z(2)), good._replace(step=z(1, 1))):
        with pytest.raises(ValueError):
            ops.keyframe_map_match(small, tab70, wrong)
    for wrong in (good._replace(key_valid=z(1, 3)), good._replace(step=z(1, dtype=torch.int64)),
                  good._replace(key_pose=z(1, 3, 3, dtype=torch.float32))):
        with pytest.raises(TypeError):
            ops.keyframe_map_match(small, tab70, wrong)
    with pytest.raises(ValueError):
        ops.keyframe_map_match(small, tab70, good, out=ops.keyframe_map_match_buffers(1, 71))
    with pytest.raises(ValueError):
        ops.keyframe_map_match(small, tab70, good, trans=z(1, 3, dtype=torch.float64))
    assert not any(t.any() for t in good)


# ------------------------------------------------------------------ 4. determinism
@pytest.mark.parametrize("N", [450, 513])
def test_the_same_bits_at_every_batch_position_in_every_run_and_in_a_graph(ops, N):
    inc, scans, poses, gates, kw, keys = shape_case(N, "gated")
    tab = ops.phi_table(inc, N)
    five = lambda a: np.repeat(a[:, :1], 5, axis=1)
    dev = Device(ops, tab, five(scans), five(poses)[0], [gates[0]] * 5, kw, keys)
    first = [dev.step(t) for t in range(T_GPU)]
    dev.reset()
    second = [dev.step(t) for t in range(T_GPU)]
    single = Device(ops, tab, scans[:, :1], poses[0, :1], gates[:1], kw, keys)
    for t in range(T_GPU):
        _same_bits(first[t], second[t], t)
        for b in range(1, 5):
            _same_bits(_sensor(first[t], 0), _sensor(first[t], b), (t, b))
        _same_bits(_sensor(first[t], 0), _sensor(single.step(t), 0), t)
    assert sum(int(f["key_switched"][0]) for f in first) == 1 and sum(int(f["key_replaced"][0]) for f in first) == 4
    # one step captured on fixed input buffers, replayed over the sequence twice with the state reset in between
    cur = torch.zeros_like(dev.scans[0])
    gate = {k: torch.zeros_like(v) for k, v in dev.gates[0].items()}
    call = lambda: ops.keyframe_map_match(cur, tab, dev.state, out=dev.out, **gate, **dev.terms, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                  # warm-up; the state it moved is reset below
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


# ------------------------------------------------------------------ 5. utils
def test_utils_keyframe_map_odometry_numpy_in_numpy_out(ops):
    import os
    import sys
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "planar_optical_flow_amd")
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    import src.utils.utils as u
    from oracle import ref_numpy as R
    inc, scans, poses, _, kw, keys = shape_case(450, "huber")
    dev = Device(ops, ops.phi_table(), scans[:, :1], poses[0, :1], None, kw, keys)
    odo = u.KeyframeMapOdometry(R.laser_phi(), keys=keys, **kw)
    odo.reset(poses[0, 0])
    for t in range(T_GPU):
        res, want = odo.update(scans[t, 0]), _sensor(dev.step(t), 0)
        for k in ("pose", "motion", "count", "rms", "iters_used", "obs", "key_age", "key_misses", "key_slot", "corr",
                  "flow_residual"):
            assert np.array_equal(np.asarray(res[k]), want[k], equal_nan=True), (t, k)
        assert np.array_equal(res["key_pose"], want["key_pose"][want["key_slot"]])
        assert isinstance(res["ok"], bool) and res["ok"] == (t > 0) and res["key_replaced"] == bool(want["key_replaced"])
        assert isinstance(res["key_switched"], bool) and res["key_switched"] == (t == 8)
    for bad in (dict(delta=1.0), dict(keys=0), dict(keys=65), dict(revisit=1.5)):
        with pytest.raises(ValueError):
            u.KeyframeMapOdometry(R.laser_phi(), **bad)


# ------------------------------------------------------------------ 6. streaming detector
STREAM = dict(method="keyframe_map", keys=KEYS_GPU, key_dist=KEY_DIST_GPU)


def test_streaming_detector_returns_to_a_stored_keyframe(ops):
    from planar_optical_flow_amd.streaming import StreamingDetector
    B = 2
    scans, poses = stream_case(B)
    T = len(scans)
    model = _stream_model(13)
    mk = lambda graph: StreamingDetector(model, batch=B, graph=graph, ego_motion=dict(STREAM))
    eager, graphed = mk(False), mk(True)
    assert eager._flow_model is None and eager._nms is None and eager._match_kw is None and not hasattr(eager, "_match_out")
    assert isinstance(eager._key_state, ops.KeyframeMapState) and eager._key_state.key_ranges.shape == (B, KEYS_GPU, 450)
    for det in (eager, graphed):
        with pytest.raises(RuntimeError):
            det.ego_motion()
        det.reset(pose=poses[0])
    with pytest.raises(ValueError):
        graphed(scans[0], pose=poses[0])
    tol, want = map_tolerance([((scans[:, b], graphed.tab.cpu().numpy(), poses[0, b], KEYS_GPU),
                                dict(MAP, key_dist=KEY_DIST_GPU)) for b in range(B)])
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
            assert_map_step_matches(_sensor(host, b), want[b][t], tol, (t, b))
            assert set(mg[b]) == {"motion", "ok", "count", "rms", "iters_used", "obs", "pose", "key_replaced", "key_age",
                                  "key_pose", "key_switched", "key_slot"}
            assert mg[b]["ok"] == (t > 0) and mg[b]["key_slot"] == int(want[b][t][1]["key_slot"])
            assert mg[b]["key_switched"] == bool(want[b][t][1]["key_switched"]) == (t == 8)
            assert np.array_equal(mg[b]["pose"], host["pose"][b])
            assert np.array_equal(mg[b]["key_pose"], host["key_pose"][b, mg[b]["key_slot"]])
    assert graphed._graph is not None and eager._graph is None
    for steps in want:
        assert_fills_evicts_and_switches(steps)
    # a new sequence from a pose of the caller's: the ring is empty again and the first scan seeds slot 0
    graphed.reset(pose=[1.0, 2.0, 0.3])
    assert not any(t.any() for t in graphed._key_state[:-1])
    graphed(dev[0])
    fit, _ = graphed.ego_motion()
    for b in range(B):
        assert not fit[b]["ok"] and fit[b]["key_replaced"] and fit[b]["key_age"] == 0 and fit[b]["key_slot"] == 0
        assert np.array_equal(fit[b]["pose"], [1.0, 2.0, 0.3]) and np.array_equal(fit[b]["key_pose"], [1.0, 2.0, 0.3])
    assert graphed._key_state.key_valid.cpu().numpy().tolist() == [[1, 0, 0]] * B


def test_streaming_settings_and_what_the_other_methods_allocate(ops):
    from planar_optical_flow_amd.streaming import StreamingDetector
    B = 2
    model, stub = _stream_model(13), _BufferFlow(B, 450).cuda()
    for kw in (dict(), dict(nms_min_dist=0.5, flow_model=stub), dict(ego_motion=dict(method="scan_match")),
               dict(nms_min_dist=0.5, flow_model=stub, ego_motion=dict(method="flow"))):
        other = StreamingDetector(model, batch=B, **kw)
        assert other._key_kw is None and not other._key_map and not hasattr(other, "_key_state"), kw
    key = StreamingDetector(model, batch=B, ego_motion=dict(method="keyframe"))
    assert isinstance(key._key_state, ops.KeyframeState) and not key._key_map and "revisit" not in key._key_kw
    for bad in (dict(method="keyframe_map", delta=1.0), dict(method="keyframe_maps"), dict(method="keyframe_map", keys=0),
                dict(method="keyframe_map", keys=65), dict(method="keyframe_map", revisit=1.5),
                dict(method="keyframe", keys=4), dict(method="keyframe", revisit=0.5)):
        with pytest.raises(ValueError):
            StreamingDetector(model, batch=B, ego_motion=bad)
    with pytest.raises(ValueError):
        StreamingDetector(model, batch=B, ego_motion=dict(method="keyframe_map"), tracks=dict())    # tracks need the flow
    det = StreamingDetector(model, batch=B, ego_motion=dict(method="keyframe_map"))
    assert det._key_state.key_ranges.shape == (B, 16, 450) and det._key_kw["revisit"] == 0.5 and "keys" not in det._key_kw
    assert {k: det._key_kw[k] for k in SETTINGS if k in ("key_dist", "key_rot", "min_share", "max_misses")} == \
        dict(key_dist=0.3, key_rot=0.3, min_share=0.5, max_misses=2)
    assert det._pose_state.data_ptr() == det._key_state.pose.data_ptr()


def test_streaming_detector_with_a_flow_model_reads_the_pose_terms_this_launch_wrote(ops):
    from planar_optical_flow_amd.streaming import StreamingDetector
    B = 1
    scans, poses = stream_case(B)
    T = len(scans)
    model, stub = _stream_model(13), _BufferFlow(B, 450).cuda()
    stub.flow.normal_(0, 0.02)
    cfg = dict(STREAM, cls_thresh=0.5)
    mk = lambda graph: StreamingDetector(model, batch=B, graph=graph, nms_min_dist=0.5, flow_model=stub, ego_motion=cfg)
    eager, graphed = mk(False), mk(True)
    assert not hasattr(graphed, "_ego_out") and not hasattr(graphed, "_match_out")
    eager.reset(pose=poses[0]), graphed.reset(pose=poses[0])
    dev = torch.from_numpy(scans).cuda()
    stored = 0
    for t in range(T):
        eager(dev[t]), graphed(dev[t])
        (me, oe), (mg, og) = eager.ego_motion(), graphed.ego_motion()
        for k in OUT:
            assert np.array_equal(getattr(oe, k).cpu().numpy(), getattr(og, k).cpu().numpy(), equal_nan=True), (t, k)
        for a, b_ in zip(eager._key_state, graphed._key_state):
            assert torch.equal(a.view(torch.uint8), b_.view(torch.uint8)), t
        stored += int(mg[0]["key_replaced"])
        pose = mg[0]["pose"]                                   # the pose terms are the pose's: the launch wrote them
        assert np.array_equal(graphed._pose_trans[0].cpu().numpy(), pose[:2])
        c, s = np.cos(pose[2]), np.sin(pose[2])
        np.testing.assert_allclose(graphed._pose_rot[0].cpu().numpy().reshape(-1), [c, -s, s, c], rtol=0, atol=1e-7)
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
    assert stored >= 2
