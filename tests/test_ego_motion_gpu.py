"""Ego-motion from a flow field (pof_ego_motion / pof_pose_advance, N6) on the GPU: against the NumPy restatement of
tests/test_ego_motion.py within the tolerance derived there, against the odometry the fixture was generated with, at
the sizes where the launch changes form, in a captured graph and as the tail of the streaming detector."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ref_numpy as R
from planar_optical_flow_amd import synth
from test_ego_motion import (ODOM_TOL_LINEAR, ODOM_TOL_RIGID, assert_matches, base_weights, fixture_odometry,
                             motion_error, rigid_field, robust_cases, tolerance, true_motion)
from test_person_flow import padded_detections

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "planar_optical_flow_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

FIELDS = ("motion", "count", "rms", "ok", "flow_residual", "weight")
CHAIN_TOL = lambda steps: 2.0 * steps * ODOM_TOL_RIGID         # per-step bound of the rigid fit, summed (x2: heading)


@pytest.fixture(scope="module")
def ops():
    from planar_optical_flow_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def u():
    import src.utils.utils as _u
    return _u


def _cuda(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _host(out):
    return {k: getattr(out, k).cpu().numpy() for k in FIELDS}


def _scan(host, b):
    return {k: v[b] for k, v in host.items()}


def _same_bits(a, b):
    for k in FIELDS:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


# ------------------------------------------------------------------ 1. fixture, exact points
def test_fixture_points_both_models_against_oracle_and_odometry(ops, u, golden):
    g = golden("scan_geometry")
    odom0, odom1 = fixture_odometry()
    xy, ones = g["xy"], np.ones(450)
    for model, name, flow, sign, tol_odom in ((0, "rigid", g["disp"], -1, ODOM_TOL_RIGID),
                                              (1, "linear", g["velocity"], 1, ODOM_TOL_LINEAR)):
        tol, want = tolerance([((xy[b], flow[b], ones, sign, model), {}) for b in range(6)])
        got = _host(ops.ego_motion(None, None, _cuda(flow), xy=_cuda(xy), canonical=False, sign=sign, model=name))
        for b in range(6):
            assert_matches(_scan(got, b), want[b], tol, (name, b))
            true = true_motion(odom0[b], odom1[b])[model]
            err = np.abs(got["motion"][b] - true).max()
            print("%s scan %d: against the odometry %.3e" % (name, b, err))
            assert err <= tol_odom
        assert np.array_equal(got["weight"], np.ones((6, 450), np.float32))
    for b in range(6):
        est = u.get_odometry_from_displacement(xy[b], g["disp"][b], odom0[b])
        assert np.abs(est - odom1[b]).max() <= ODOM_TOL_RIGID, (b, est - odom1[b])
        est = u.get_odometry_from_velocity(xy[b], g["velocity"][b], odom0[b])
        assert np.abs(est - odom1[b]).max() <= ODOM_TOL_LINEAR, (b, est - odom1[b])


# ------------------------------------------------------------------ 2. ranges + canonical float32
def test_ranges_and_canonical_float32_flow(ops, golden):
    g = golden("scan_geometry")
    scans = synth.make_batch(seed=1, B=6, T=2, mixed_classes=True).scans[:, -1]
    odom0, odom1 = fixture_odometry()
    tab = ops.phi_table()
    phi = tab[:450].cpu().numpy()
    flow = _cuda(g["disp_canonical"], np.float32)
    f = ops.rotate_flow(flow, tab, False).cpu().numpy().astype(np.float64)     # the device's own scanner-frame flow
    p = np.stack(R.polar_to_xy(scans, phi[None]), axis=2)
    w0 = [base_weights(p[b], f[b], ranges=scans[b]) for b in range(6)]
    assert any((w < 1).any() for w in w0)                                      # the 29.99 dropouts are gated
    tol, want = tolerance([((p[b], f[b], w0[b], -1, 0), {}) for b in range(6)])
    got = _host(ops.ego_motion(_cuda(scans), tab, flow))
    for b in range(6):
        assert_matches(_scan(got, b), want[b], tol, b)
        assert np.array_equal(got["weight"][b], w0[b].astype(np.float32))
        # float32 flow: 2^-24 * 0.07 m per point, far inside the bound of the reference's float32 matrices
        assert np.abs(got["motion"][b] - true_motion(odom0[b], odom1[b])[0]).max() <= ODOM_TOL_RIGID
    # without the range gate the dropouts count again
    assert (_host(ops.ego_motion(_cuda(scans), tab, flow, max_range=30.0))["count"] == 450).all()


# ------------------------------------------------------------------ 3. gates
def test_gates_weights_nonfinite_flow_and_detections(ops, golden):
    g = golden("person_flow")
    B, N = g["inst"].shape
    scans = g["scans"].astype(np.float32)
    tab = ops.phi_table()
    phi = tab[:N].cpu().numpy()
    rng = np.random.default_rng(17)
    flow = g["flow"].copy()
    bad = [3, 77, 200, 201, 449]
    flow[0, bad[0], 0] = np.nan
    flow[0, bad[1], 1] = np.inf
    flow[1, bad[2]] = -np.inf
    flow[1, bad[3], 1] = np.nan
    flow[2, bad[4]] = np.nan
    weight = rng.uniform(0.2, 2.0, (B, N)).astype(np.float32)
    weight[:, 10:20] = 0.0
    weight[:, 30:35] = -1.0
    weight[1, 40] = np.nan
    weight[2, 41] = np.inf
    det_cls = np.stack([padded_detections(g, b)[1] for b in range(B)])
    f = ops.rotate_flow(_cuda(flow), tab, False).cpu().numpy().astype(np.float64)
    p = np.stack(R.polar_to_xy(scans, phi[None]), axis=2)
    counts = {}
    for thresh in (0.5, 2.0):
        w0 = [base_weights(p[b], f[b], weight=weight[b], ranges=scans[b], inst=g["inst"][b], num=g["num"][b],
                           det_cls=det_cls[b], cls_thresh=thresh) for b in range(B)]
        tol, want = tolerance([((p[b], f[b], w0[b], -1, 0), {}) for b in range(B)])
        got = _host(ops.ego_motion(_cuda(scans), tab, _cuda(flow), weight=_cuda(weight), instance_mask=_cuda(g["inst"], np.int32),
                                   num_det=_cuda(g["num"], np.int32), det_cls=_cuda(det_cls), cls_thresh=thresh))
        for b in range(B):
            assert_matches(_scan(got, b), want[b], tol, (thresh, b))
            assert np.isfinite(got["motion"][b]).all()
            assert np.array_equal(got["weight"][b] == 0, w0[b] == 0)
            assert np.array_equal(got["weight"][b], w0[b].astype(np.float32))
        counts[thresh] = got["count"]
    # at 2.0 no detection is a person: only the ranges, the weights and the flow gate
    no_det = [base_weights(p[b], f[b], weight=weight[b], ranges=scans[b]).astype(bool).sum() for b in range(B)]
    assert np.array_equal(counts[2.0], no_det) and (counts[0.5] < counts[2.0]).all()


# ------------------------------------------------------------------ 4. robust fit
def test_huber_passes_halve_the_error_of_the_plain_fit(ops):
    cases = robust_cases(8)
    xy = np.stack([c[0] for c in cases])
    disp = np.stack([c[1] for c in cases])
    ones = np.ones(xy.shape[1])
    kw = dict(huber_delta=0.02, iters=4)
    tol, want = tolerance([((xy[b], disp[b].astype(np.float64), ones, -1, 0), kw) for b in range(8)])
    args = dict(xy=_cuda(xy), canonical=False)
    robust = _host(ops.ego_motion(None, None, _cuda(disp), **args, **kw))
    plain = _host(ops.ego_motion(None, None, _cuda(disp), **args))
    for b in range(8):
        assert_matches(_scan(robust, b), want[b], tol, b)
        np.testing.assert_allclose(robust["weight"][b], want[b]["weight"], rtol=1e-6, atol=0)
        e_plain, e_robust = (motion_error(r["motion"][b], cases[b][2]) for r in (plain, robust))
        print("scan %d: plain %.3e robust %.3e ratio %.2f" % (b, e_plain, e_robust, e_plain / e_robust))
        assert e_robust <= 0.5 * e_plain


# ------------------------------------------------------------------ 5. sizes and forms
def _sized(N, B=3, seed=0):
    rng = np.random.default_rng(1000 + N + seed)
    xy = rng.normal(0, 5, (B, N, 2))
    flow = np.stack([rigid_field(xy[b], rng.uniform(-0.03, 0.03), rng.uniform(-0.05, 0.05, 2)) for b in range(B)])
    flow += rng.normal(0, 0.01, flow.shape)
    weight = rng.uniform(0.5, 1.5, (B, N)).astype(np.float32)
    if N > 8:
        weight[:, ::7] = 0.0
    return xy, flow, weight


@pytest.mark.parametrize("N", [2, 64, 65, 450, 512, 513, 3600, 4096])
def test_wave_and_workgroup_forms_at_their_sizes(ops, N):
    """N <= 512 is the one-wave form (a partial last slot at 65 and 450, full slots at 64 and 512), 513 the workgroup
    form with one point in its second wave, 3600 and 4096 fill it."""
    xy, flow, weight = _sized(N)
    kw = dict(huber_delta=0.01, iters=2)
    for model, name in ((0, "rigid"), (1, "linear")):
        cases = [((xy[b], flow[b], base_weights(xy[b], flow[b], weight=weight[b]), -1, model), kw) for b in range(3)]
        tol, want = tolerance(cases)
        got = _host(ops.ego_motion(None, None, _cuda(flow), xy=_cuda(xy), canonical=False, model=name,
                                   weight=_cuda(weight), **kw))
        for b in range(3):
            assert_matches(_scan(got, b), want[b], tol, (name, b))
            assert got["ok"][b] == 1


def test_degenerate_scans_and_limits(ops):
    from planar_optical_flow_amd._lib import POF_E_SHAPE, PofError
    run = lambda xy, flow, **kw: _host(ops.ego_motion(None, None, _cuda(flow), xy=_cuda(xy), canonical=False, **kw))
    p2 = np.array([[[1.0, 2.0], [-3.0, 0.5]]])
    two = run(p2, rigid_field(p2[0], 0.02, (0.04, -0.03))[None])
    assert two["ok"][0] == 1 and two["rms"][0] <= 1e-12 and two["count"][0] == 2
    np.testing.assert_allclose(two["motion"][0], [0.02, 0.04, -0.03], rtol=0, atol=1e-12)
    one = run(p2[:, :1], np.zeros((1, 1, 2)))
    assert one["ok"][0] == 0 and np.isnan(one["motion"]).all() and one["count"][0] == 1 and np.isnan(one["rms"][0])
    xy, flow, _ = _sized(70)
    none = run(xy, flow, weight=_cuda(np.zeros((3, 70), np.float32)))
    assert not none["ok"].any() and not none["count"].any() and np.isnan(none["motion"]).all() and not none["weight"].any()
    same = run(np.ones((3, 70, 2)), flow)
    assert not same["ok"].any() and (same["count"] == 70).all() and np.isnan(same["motion"]).all()
    with pytest.raises(PofError) as e:
        run(np.zeros((1, 4097, 2)), np.zeros((1, 4097, 2)))
    assert e.value.code == POF_E_SHAPE
    empty = ops.ego_motion(None, None, torch.zeros(0, 70, 2, dtype=torch.float64, device="cuda"),
                           xy=torch.zeros(0, 70, 2, dtype=torch.float64, device="cuda"), canonical=False)
    assert empty.motion.shape == (0, 3) and empty.flow_residual.shape == (0, 70, 2) and empty.ok.shape == (0,)
    with pytest.raises(ValueError):
        ops.ego_motion(None, None, _cuda(flow), xy=_cuda(xy), canonical=False, out=ops.ego_motion_buffers(3, 71))
    with pytest.raises(ValueError):
        ops.ego_motion(None, None, _cuda(flow), xy=_cuda(xy))          # a canonical flow needs the table
    out = ops.ego_motion_buffers(3, 70)
    assert ops.ego_motion(None, None, _cuda(flow), xy=_cuda(xy), canonical=False, out=out).rms.data_ptr() == out.rms.data_ptr()


@pytest.mark.parametrize("N", [450, 513])
def test_a_scan_gives_the_same_bits_at_every_batch_position_and_in_every_run(ops, N):
    xy, flow, weight = _sized(N, B=70, seed=5)
    xy[69], flow[69], weight[69] = xy[0], flow[0], weight[0]
    kw = dict(canonical=False, huber_delta=0.01, iters=3)
    run = lambda sl: _host(ops.ego_motion(None, None, _cuda(flow[sl]), xy=_cuda(xy[sl]), weight=_cuda(weight[sl]), **kw))
    batch, alone, again = run(slice(None)), run(slice(0, 1)), run(slice(None))
    _same_bits(_scan(batch, 0), _scan(batch, 69))
    _same_bits(_scan(batch, 0), _scan(alone, 0))
    _same_bits(batch, again)
    assert not np.array_equal(batch["motion"][0], batch["motion"][1])


# ------------------------------------------------------------------ 6. pose_advance
def _advance(pose, motion, ok):
    """NumPy statement of pof_pose_advance -> (pose1, rot float32 [B,4], trans, flow_trans)."""
    pose1 = pose.copy()
    c, s = np.cos(pose[:, 2]), np.sin(pose[:, 2])
    k = ok.astype(bool)
    pose1[k, 0] = pose[k, 0] + (c[k] * motion[k, 1] - s[k] * motion[k, 2])
    pose1[k, 1] = pose[k, 1] + (s[k] * motion[k, 1] + c[k] * motion[k, 2])
    pose1[k, 2] = pose[k, 2] + motion[k, 0]
    c1, s1 = np.cos(pose1[:, 2]), np.sin(pose1[:, 2])
    return pose1, np.stack([c1, -s1, s1, c1], axis=1).astype(np.float32), pose1[:, :2].copy(), pose1[:, :2] - pose[:, :2]


def test_pose_advance_against_numpy(ops):
    rng = np.random.default_rng(23)
    B = 5
    pose = np.concatenate([rng.uniform(-100, 100, (B, 2)), rng.uniform(-np.pi, np.pi, (B, 1))], axis=1)
    motion = np.concatenate([rng.uniform(-0.03, 0.03, (B, 1)), rng.uniform(-0.05, 0.05, (B, 2))], axis=1)
    ok = np.array([1, 1, 0, 1, 1], np.uint8)
    motion[2] = np.nan                                              # what a failed fit leaves
    want_pose, want_rot, want_trans, want_ftr = _advance(pose, motion, ok)
    dev = _cuda(pose)
    rot = torch.zeros(B, 2, 2, device="cuda")
    trans, ftr = (torch.zeros(B, 2, dtype=torch.float64, device="cuda") for _ in range(2))
    assert ops.pose_advance(_cuda(motion), _cuda(ok), dev, rot, trans, ftr) is dev
    got = dev.cpu().numpy()
    np.testing.assert_allclose(got, want_pose, rtol=0, atol=1e-12)
    np.testing.assert_allclose(trans.cpu().numpy(), want_trans, rtol=0, atol=1e-12)
    np.testing.assert_allclose(ftr.cpu().numpy(), want_ftr, rtol=0, atol=1e-12)
    got_rot = rot.cpu().numpy().reshape(B, 4)
    assert np.all(np.abs(got_rot - want_rot) <= np.spacing(np.abs(want_rot)))          # one float32 ulp
    assert np.array_equal(got[2], pose[2]) and not ftr.cpu().numpy()[2].any()
    assert np.array_equal(trans.cpu().numpy()[2], pose[2, :2])
    # the three pose-term outputs are optional
    alone = _cuda(pose)
    ops.pose_advance(_cuda(motion), _cuda(ok), alone)
    assert np.array_equal(alone.cpu().numpy(), got)
    with pytest.raises(ValueError):
        ops.pose_advance(_cuda(motion), _cuda(ok[:4]), _cuda(pose))


def test_dead_reckoning_over_twenty_steps(ops):
    rng = np.random.default_rng(29)
    T, N = 20, 450
    phi = R.laser_phi()
    steps = np.concatenate([rng.uniform(-0.05, 0.05, (T, 2)), rng.uniform(-0.03, 0.03, (T, 1))], axis=1)
    start = np.array([3.0, -2.0, 0.7])
    poses = np.concatenate([start[None], start + np.cumsum(steps, axis=0)])
    r = np.clip(6 + 3 * np.sin(2 * phi + 1.0) + 1.5 * np.sin(7 * phi + 2.0), 0.3, 25)
    xy = np.stack(R.polar_to_xy(r, phi), axis=1)
    disp = np.stack([R.displacement_from_odometry(xy, poses[t], poses[t + 1]) for t in range(T)])
    fit = ops.ego_motion(None, None, _cuda(disp), xy=_cuda(np.broadcast_to(xy, (T, N, 2))), canonical=False)
    pose = _cuda(start[None])
    for t in range(T):
        ops.pose_advance(fit.motion[t:t + 1], fit.ok[t:t + 1], pose)
    err = np.abs(pose.cpu().numpy()[0] - poses[-1])
    print("dead reckoning over %d steps: %.3e m %.3e rad" % (T, err[:2].max(), err[2]))
    assert err.max() <= CHAIN_TOL(T)


# ------------------------------------------------------------------ 7. graph
def test_captured_fit_and_pose_replay_bit_identically(ops):
    B, N = 2, 450
    cases = robust_cases(8, seed=41)
    xy_in = torch.zeros(B, N, 2, dtype=torch.float64, device="cuda")
    flow_in = torch.zeros(B, N, 2, dtype=torch.float32, device="cuda")
    kw = dict(canonical=False, huber_delta=0.02, iters=4)
    mk = lambda: (ops.ego_motion_buffers(B, N), torch.zeros(B, 3, dtype=torch.float64, device="cuda"),
                  torch.zeros(B, 2, 2, device="cuda"), torch.zeros(B, 2, dtype=torch.float64, device="cuda"),
                  torch.zeros(B, 2, dtype=torch.float64, device="cuda"))

    def step(bufs):
        out, pose, rot, trans, ftr = bufs
        ops.ego_motion(None, None, flow_in, xy=xy_in, out=out, **kw)
        ops.pose_advance(out.motion, out.ok, pose, rot, trans, ftr)

    captured, eager = mk(), mk()
    xy_in.copy_(_cuda(np.stack([cases[6][0], cases[7][0]])))
    flow_in.copy_(_cuda(np.stack([cases[6][1], cases[7][1]])))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(mk())                                                  # warm-up on buffers of its own
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(captured)
    for r in range(3):
        xy_in.copy_(_cuda(np.stack([cases[2 * r][0], cases[2 * r + 1][0]])))
        flow_in.copy_(_cuda(np.stack([cases[2 * r][1], cases[2 * r + 1][1]])))
        graph.replay()
        step(eager)
        _same_bits(_host(captured[0]), _host(eager[0]))
        for a, b in zip(captured[1:], eager[1:]):
            assert torch.equal(a, b)
        assert captured[0].ok.all() and captured[1].abs().sum() > 0


# ------------------------------------------------------------------ 8. streaming detector
class _BufferFlow(torch.nn.Module):
    """A 'flow net' that returns a registered buffer the test fills: (previous scan, scan) [B,N,1] -> [B,N,2]."""

    def __init__(self, B, N):
        super().__init__()
        self.register_buffer("flow", torch.zeros(B, N, 2))

    def forward(self, prev, cur):
        return self.flow


def _stream_model(seed):
    from planar_optical_flow_amd.src.depracted.model.dr_spaam import SpatialDROW
    torch.manual_seed(seed)
    return SpatialDROW(num_scans=5, num_pts=56, alpha=0.5, window_size=11, pedestrian_only=True).cuda().eval()


def _sequence(B, T, seed):
    """Scans [B,T,450], true poses [T,B,3] and the canonical float32 displacement field of every step [T,B,450,2]
    (zeros at t = 0)."""
    scans = synth.make_batch(seed=seed, B=B, T=T).scans
    rng = np.random.default_rng(seed + 1)
    steps = np.concatenate([rng.uniform(-0.05, 0.05, (T, B, 2)), rng.uniform(-0.03, 0.03, (T, B, 1))], axis=2)
    poses = np.cumsum(steps, axis=0) + np.array([60.0, 100.0, 0.4])
    phi = R.laser_phi()
    flows = np.zeros((T, B, 450, 2), np.float32)
    for t in range(1, T):
        for b in range(B):
            xy = np.stack(R.polar_to_xy(scans[b, t], phi), axis=1)
            flows[t, b] = R.flow_to_canonical(R.displacement_from_odometry(xy, poses[t - 1, b], poses[t, b]), phi)
    return torch.from_numpy(scans).cuda(), poses, torch.from_numpy(flows).cuda()


def _same_results(a, b, atol=None):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for k in x:
            if atol is None or x[k].dtype.kind != "f":
                assert np.array_equal(x[k], y[k], equal_nan=True), k
            else:
                assert np.array_equal(np.isnan(x[k]), np.isnan(y[k])), k
                np.testing.assert_allclose(x[k], y[k], rtol=0, atol=atol, err_msg=k)


@pytest.mark.parametrize("B", [1, 2])
def test_streaming_detector_dead_reckons_its_own_pose(B):
    from planar_optical_flow_amd.streaming import StreamingDetector
    T = 5
    model, stub = _stream_model(13), _BufferFlow(B, 450).cuda()
    scans, poses, flows = _sequence(B, T, seed=51 + B)
    ego = dict(huber_delta=0.02, iters=4, max_range=20.0, cls_thresh=2.0)     # the random net's detections gate nothing
    mk = lambda graph, **kw: StreamingDetector(model, batch=B, graph=graph, nms_min_dist=0.5, flow_model=stub, **kw)
    eager, graphed, posed = mk(False, ego_motion=ego), mk(True, ego_motion=ego), mk(True)
    eager.reset(pose=poses[0]), graphed.reset(pose=poses[0])
    with pytest.raises(ValueError):
        graphed(scans[:, 0], pose=poses[0])
    for t in range(T):
        stub.flow.copy_(flows[t])
        eager(scans[:, t]), graphed(scans[:, t])
        if t == 0:
            for det in (eager, graphed):
                with pytest.raises(RuntimeError):
                    det.ego_motion()
            posed(scans[:, 0], pose=poses[0])
            continue
        (me, oe), (mg, og) = eager.ego_motion(), graphed.ego_motion()
        _same_results(me_arrays(me), me_arrays(mg))
        for k in FIELDS:
            assert np.array_equal(getattr(oe, k).cpu().numpy(), getattr(og, k).cpu().numpy(), equal_nan=True), k
        (pe, fe), (pg, fg) = eager.person_flow(), graphed.person_flow()
        _same_results(pe, pg)
        for k in fe._fields:
            assert np.array_equal(getattr(fe, k).cpu().numpy(), getattr(fg, k).cpu().numpy(), equal_nan=True), k
        est = np.stack([m["pose"] for m in mg])
        err = np.abs(est - poses[t])
        print("B=%d t=%d: dead-reckoned pose error %.3e m %.3e rad, count %s" % (B, t, err[:, :2].max(), err[:, 2].max(),
                                                                          [m["count"] for m in mg]))
        assert all(m["ok"] for m in mg) and err.max() <= CHAIN_TOL(t)
        # the same per-person flow as a detector that is handed those poses
        posed(scans[:, t], pose=est)
        _same_results(posed.person_flow()[0], pg, atol=1e-6)
    assert graphed._graph is not None and eager._graph is None
    # a new sequence from a pose of the caller's
    start = np.array([-7.0, 2.5, -1.1])
    graphed.reset(pose=start)
    stub.flow.copy_(flows[0])
    graphed(scans[:, 0])
    assert np.array_equal(graphed._pose_state.cpu().numpy(), np.broadcast_to(start, (B, 3)))
    with pytest.raises(RuntimeError):
        graphed.ego_motion()
    stub.flow.copy_(flows[1])
    graphed(scans[:, 1])
    fit, _ = graphed.ego_motion()
    for b in range(B):
        want = _advance(start[None], fit[b]["motion"][None], np.ones(1, np.uint8))[0][0]
        np.testing.assert_allclose(fit[b]["pose"], want, rtol=0, atol=1e-12)
        np.testing.assert_allclose(fit[b]["motion"], true_motion(poses[0, b], poses[1, b])[0], rtol=0, atol=ODOM_TOL_RIGID)


def me_arrays(fits):
    return [{k: np.asarray(v) for k, v in m.items()} for m in fits]


def test_streaming_detector_gates_its_own_confident_detections():
    from planar_optical_flow_amd.streaming import StreamingDetector
    B = 2
    model, stub = _stream_model(13), _BufferFlow(B, 450).cuda()
    scans, poses, flows = _sequence(B, 2, seed=57)
    det = StreamingDetector(model, batch=B, nms_min_dist=0.5, flow_model=stub, ego_motion=dict())
    for t in range(2):
        stub.flow.copy_(flows[t])
        det(scans[:, t])
    fits, out = det.ego_motion()
    dets, inst = det.detections()
    r = scans[:, 1].cpu().numpy()
    for b in range(B):
        conf = dets[b][1]
        ids = inst[b]
        member = (ids >= 1) & (ids <= len(conf))
        person = np.zeros(450, bool)
        person[member] = conf[ids[member] - 1] >= 0.5
        want = int((~person & (r[b] < 20.0)).sum())
        assert fits[b]["count"] == want and np.array_equal(out.weight[b].cpu().numpy() > 0, ~person & (r[b] < 20.0))
    with pytest.raises(ValueError):
        StreamingDetector(model, batch=B, nms_min_dist=0.5, ego_motion=dict())       # the motion is fitted to a flow
    with pytest.raises(ValueError):
        StreamingDetector(model, batch=B, nms_min_dist=0.5, flow_model=stub, ego_motion=dict(delta=1.0))
    plain = StreamingDetector(model, batch=B, nms_min_dist=0.5, flow_model=stub)
    for name in ("_ego_out", "_pose_state"):
        assert not hasattr(plain, name), name
    with pytest.raises(ValueError):
        plain.reset(pose=poses[0])
