"""Per-person flow (pof_person_flow, N5) on the GPU: against the reference's results within the bounds derived in
tests/test_person_flow.py, against the device's own per-point outputs bit for bit, at the sizes where the launch
changes form, and as the tail of the streaming detector's captured step."""
import os
import sys

import numpy as np
import pytest
import torch

from planar_optical_flow_amd import synth
from test_person_flow import (CLS_THRESH, assert_within_golden_bounds, padded_detections, pose_terms,
                              restate_flow_global, restate_flow_world, sequential_means)

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "planar_optical_flow_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

FIELDS = ("flow_global", "flow_world", "rgb", "det_xy_world", "det_flow", "det_rgb", "det_count", "det_valid")


@pytest.fixture(scope="module")
def ops():
    from planar_optical_flow_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def u():
    import src.utils.utils as _u
    return _u


def _cuda(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _host(out):
    return {k: getattr(out, k).cpu().numpy() for k in FIELDS}


@pytest.fixture(scope="module")
def fixture_run(ops, golden):
    """ops.person_flow on the fixture's own NMS results (all four scans in one launch), computed once."""
    g = golden("person_flow")
    B, N = g["inst"].shape
    xy, cl = np.zeros((B, N, 2)), np.zeros((B, N))
    rot, trans, ftr = np.zeros((B, 2, 2), np.float32), np.zeros((B, 2)), np.zeros((B, 2))
    for b in range(B):
        xy[b], cl[b], _ = padded_detections(g, b)
        rot[b], trans[b], ftr[b] = pose_terms(g, b)
    args = (_cuda(g["flow"]), ops.phi_table(), _cuda(g["inst"], np.int32), _cuda(g["num"], np.int32), _cuda(xy),
            _cuda(cl), _cuda(rot), _cuda(trans), _cuda(ftr), CLS_THRESH)
    out = ops.person_flow(*args)
    torch.cuda.synchronize()
    return g, args, out


# ------------------------------------------------------------------ 1. golden, decoupled from the NMS
def test_golden_results_within_the_derived_bounds(ops, fixture_run):
    g, args, out = fixture_run
    got = _host(out)
    exact_global = ops.rotate_flow(args[0], args[1], False).cpu().numpy()
    for b in range(4):
        assert_within_golden_bounds({k: v[b] for k, v in got.items()}, g, b, exact_global=exact_global[b])


# ------------------------------------------------------------------ 2. exact layer
def test_colour_and_sums_are_exact_on_the_devices_own_outputs(ops, u, fixture_run):
    g, args, out = fixture_run
    got = _host(out)
    # the colour code of the device's own world flow: the project's tolerance for flow_to_hsv
    np.testing.assert_allclose(got["rgb"], u.flow_to_hsv(got["flow_world"]), rtol=0, atol=1e-12)
    # sequential float64 sums in point order, divided by the count: bit for bit
    for b in range(4):
        for name, src in (("det_flow", "flow_world"), ("det_rgb", "rgb")):
            want, count = sequential_means(g["inst"][b], g["num"][b], got[src][b])
            assert np.array_equal(got[name][b], want, equal_nan=True), (name, b)
            assert np.array_equal(got["det_count"][b], count)
    # two runs: identical buffers
    again = _host(ops.person_flow(*args))
    for k in FIELDS:
        assert np.array_equal(got[k], again[k], equal_nan=True), k


def test_zero_flow_without_translation_is_exactly_white(ops):
    B, N = 2, 130
    rot = np.stack([pose_terms({"odom1": [np.array([1.0, 2.0, 0.7])], "odom0": [np.array([1.0, 2.0, 0.1])]}, 0)[0]] * B)
    inst = (np.arange(B * N).reshape(B, N) % 4).astype(np.int32)
    out = ops.person_flow(torch.zeros(B, N, 2, device="cuda"), ops.phi_table(num_pts=N), _cuda(inst),
                          _cuda(np.array([3, 3], np.int32)), torch.zeros(B, N, 2, dtype=torch.float64, device="cuda"),
                          torch.ones(B, N, dtype=torch.float64, device="cuda"), _cuda(rot))
    got = _host(out)
    assert np.array_equal(got["rgb"], np.ones((B, N, 3))) and not got["flow_world"].any()
    assert np.array_equal(got["det_rgb"][:, :3], np.ones((B, 3, 3))) and not got["det_rgb"][:, 3:].any()
    assert not got["det_flow"].any()


def test_nan_flow_takes_numpys_sector(ops):
    """A NaN flow has no hue: NumPy's int64 cast of NaN is INT64_MIN, sector 4 = (t, p, v) -> (NaN, NaN, 1), and
    the NaN stays inside its own instance's means."""
    N = 70
    flow = np.zeros((1, N, 2), np.float32)
    flow[0, 5, 0] = np.nan
    inst = np.ones((1, N), np.int32)
    inst[0, 5] = 2
    got = _host(ops.person_flow(_cuda(flow), ops.phi_table(num_pts=N), _cuda(inst), _cuda(np.array([2], np.int32)),
                                torch.zeros(1, N, 2, dtype=torch.float64, device="cuda"),
                                torch.ones(1, N, dtype=torch.float64, device="cuda")))
    assert np.array_equal(got["rgb"][0, 5], [np.nan, np.nan, 1.0], equal_nan=True)
    assert np.array_equal(np.delete(got["rgb"][0], 5, axis=0), np.ones((N - 1, 3)))
    assert np.array_equal(got["det_rgb"][0, :2], [[1.0, 1.0, 1.0], [np.nan, np.nan, 1.0]], equal_nan=True)
    assert np.isnan(got["det_flow"][0, 1]).all() and not got["det_flow"][0, 0].any()


# ------------------------------------------------------------------ 3. end to end
def test_reference_shaped_function_reproduces_the_fixture(u, golden):
    g = golden("person_flow")
    phi = u.get_laser_phi()
    N = g["inst"].shape[1]
    for b in range(4):
        res = u.person_flow(g["scans"][b], phi, g["cls"][b], g["reg"][b], g["flow"][b], g["odom1"][b], g["odom0"][b])
        _, _, sl = padded_detections(g, b)
        m = int(g["num"][b])
        # masks, scores and counts are reproduced exactly.  The centres are the NMS's: the project holds them to
        # 1e-12 of the reference (its sincos / atan2 are the device's), so they are compared after the world
        # transform within the centre bound here, and directly at that tolerance in the scanner-frame call below
        assert np.array_equal(res["instance_mask"], g["inst"][b]) and res["instance_mask"].dtype == np.int32
        assert np.array_equal(res["dets_cls"], g["dets_cls"][sl].reshape(-1, 1)) and len(res["count"]) == m
        assert res["valid"].dtype == np.bool_ and res["person_flow"].shape == (m, 2) and res["person_rgb"].shape == (m, 3)
        pad = lambda a: np.concatenate([a, np.zeros((N - m,) + a.shape[1:], a.dtype)])
        got = {"flow_world": res["flow_world"], "rgb": res["rgb"], "det_xy_world": pad(res["dets_xy_world"]),
               "det_flow": pad(res["person_flow"]), "det_rgb": pad(res["person_rgb"]), "det_count": pad(res["count"]),
               "det_valid": pad(res["valid"])}
        assert_within_golden_bounds(got, g, b)
    # scanner frame: no pose, nothing added
    res = u.person_flow(g["scans"][0], phi, g["cls"][0], g["reg"][0], g["flow"][0])
    assert np.array_equal(res["flow_world"], u.canonical_to_global_flow_torch(g["flow"][0], phi).astype(np.float64))
    np.testing.assert_allclose(res["dets_xy_world"], g["dets_xy"][:int(g["num"][0])], rtol=0, atol=1e-12)   # the NMS's own


# ------------------------------------------------------------------ 4. shapes where it can go wrong
def _table(N):
    """An angle table [3N] built by hand (pof_laser_phi needs two points): phi | (cos, sin) interleaved."""
    phi = np.linspace(-1.9, 1.9, N) if N > 1 else np.array([0.3])
    return phi, np.concatenate([phi, np.stack([np.cos(phi), np.sin(phi)], axis=1).reshape(-1)])


def _synthetic(N, seed):
    """B = 3 scans with synthetic masks.  Scan 0: one instance owns every point.  Scan 1: every point its own
    instance, in a shuffled order (num_det = N).  Scan 2: ids drawn from [0, nd + 2] with num_det = nd -- id 0, one
    negative id and ids above num_det occur, and id 2 never does (an instance without points)."""
    rng = np.random.default_rng(seed)
    inst = np.zeros((3, N), np.int32)
    inst[0] = 1
    inst[1] = rng.permutation(N) + 1
    nd = max(1, min(N, 70) // 2 + 1) if N > 1 else 1
    ids = rng.integers(0, nd + 3, N)
    ids[ids == 2] = 3 if nd >= 3 else 0
    if N >= 8:
        ids[:5] = (0, nd + 1, nd + 2, 1, 3)
        ids[5] = -3
    inst[2] = ids
    num = np.array([1, N, nd], np.int32)
    flow = rng.normal(0, 0.05, (3, N, 2)).astype(np.float32)
    flow[:, ::7] = 0.0
    det_xy = rng.normal(0, 5.0, (3, N, 2))
    det_cls = rng.uniform(0.0, 1.0, (3, N))
    det_cls[2, 0] = CLS_THRESH                                   # equality counts as valid
    if nd > 1 or N > 1:
        det_cls[1, min(1, N - 1)] = np.nextafter(CLS_THRESH, 0.0)    # the float64 below it does not
    poses = rng.uniform(-3, 3, (3, 2, 3))
    from planar_optical_flow_amd.src.utils.utils import _pose_terms
    rot, trans, ftr = _pose_terms(poses[:, 1], poses[:, 0])
    return inst, num, flow, det_xy, det_cls, rot, trans, ftr


@pytest.mark.parametrize("N", [1, 64, 65, 450, 512, 513, 577])
def test_wave_and_workgroup_forms_at_their_sizes(ops, u, N):
    """N <= 512 is the one-wave form (partial last column at 65 and 450, full columns at 64 and 512), 513 the
    workgroup form with a second chunk of one point, 577 with a second chunk of 65: a wave's walk takes one full group
    of 64 staged points and a group of one."""
    inst, num, flow, det_xy, det_cls, rot, trans, ftr = _synthetic(N, 40 + N)
    phi, tab = _table(N)
    args = (_cuda(flow), _cuda(tab), _cuda(inst), _cuda(num), _cuda(det_xy), _cuda(det_cls), _cuda(rot), _cuda(trans),
            _cuda(ftr), CLS_THRESH)
    got = _host(ops.person_flow(*args))
    assert np.array_equal(got["flow_global"], ops.rotate_flow(args[0], args[1], False).cpu().numpy())
    np.testing.assert_allclose(got["rgb"], u.flow_to_hsv(got["flow_world"]), rtol=0, atol=1e-12)
    for b in range(3):
        nd = int(num[b])
        g32 = restate_flow_global(flow[b], phi)
        assert np.array_equal(got["flow_global"][b], g32)
        f = np.abs(flow[b].astype(np.float64)).sum(axis=1)
        assert np.all(np.abs(got["flow_world"][b] - restate_flow_world(g32, rot[b], ftr[b])).max(axis=1) <= 2.0 ** -19 * f)
        for name, src in (("det_flow", "flow_world"), ("det_rgb", "rgb")):
            want, count = sequential_means(inst[b], nd, got[src][b])
            assert np.array_equal(got[name][b], want, equal_nan=True), (name, b)
            assert np.array_equal(got["det_count"][b], count), b
        rd = rot[b].astype(np.float64)
        want_xy = np.stack([(det_xy[b, :nd, 1] * rd[c, 1] + det_xy[b, :nd, 0] * rd[c, 0]) + trans[b, c] for c in (0, 1)], 1)
        bound = 2.0 ** -50 * (np.abs(det_xy[b, :nd]).sum(axis=1)[:, None] + np.abs(trans[b])[None, :])
        assert np.all(np.abs(got["det_xy_world"][b, :nd] - want_xy) <= bound)
        assert np.array_equal(got["det_valid"][b, :nd], (det_cls[b, :nd] >= CLS_THRESH).astype(np.uint8))
        for name in FIELDS[3:]:
            assert not got[name][b, nd:].any(), (name, b)          # rows k >= num_det are zero
    assert got["det_count"][0, 0] == N and np.array_equal(got["det_count"][1], np.ones(N, np.int32))
    assert np.array_equal(got["det_flow"][1][inst[1] - 1], got["flow_world"][1])     # one point each: its own flow
    assert got["det_valid"][2, 0] == 1
    if N > 1:
        assert got["det_valid"][1, 1] == 0
    if num[2] >= 3:                                                   # the instance without points
        assert got["det_count"][2, 1] == 0 and np.isnan(got["det_flow"][2, 1]).all() and np.isnan(got["det_rgb"][2, 1]).all()
        assert np.isfinite(got["det_flow"][2, [0, 2]]).all() and np.isfinite(got["det_rgb"][2, [0, 2]]).all()
    # num_det = 0 (and a count outside [0, N], which is clamped): all-zero per-detection buffers
    none = _host(ops.person_flow(*args[:3], _cuda(np.array([0, -5, 0], np.int32)), *args[4:]))
    for name in FIELDS[3:]:
        assert not none[name].any(), name
    for name in FIELDS[:3]:
        assert np.array_equal(none[name], got[name]), name
    over = _host(ops.person_flow(*args[:3], _cuda(np.array([1, N + 9, num[2]], np.int32)), *args[4:]))
    for name in FIELDS:
        assert np.array_equal(over[name], got[name], equal_nan=True), name


def test_argument_checks(ops):
    from planar_optical_flow_amd._lib import POF_E_SHAPE, PofError
    dev = "cuda"
    mk = lambda B, N: (torch.zeros(B, N, 2, device=dev), torch.zeros(3 * N, dtype=torch.float64, device=dev),
                       torch.zeros(B, N, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev),
                       torch.zeros(B, N, 2, dtype=torch.float64, device=dev),
                       torch.zeros(B, N, dtype=torch.float64, device=dev))
    with pytest.raises(PofError) as e:
        ops.person_flow(*mk(1, 4097))
    assert e.value.code == POF_E_SHAPE
    assert ops.person_flow(*mk(1, 4096)).det_count.shape == (1, 4096)
    with pytest.raises(TypeError):
        ops.person_flow(*(t.cpu() for t in mk(2, 8)))
    with pytest.raises(TypeError):
        ops.person_flow(*mk(2, 8), rot=torch.eye(2).repeat(2, 1, 1))                     # a CPU pose
    with pytest.raises(ValueError):
        ops.person_flow(*mk(2, 8), rot=torch.zeros(2, 3, 3, device=dev))
    with pytest.raises(ValueError):
        ops.person_flow(*mk(2, 8), trans=torch.zeros(2, 3, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        ops.person_flow(*mk(2, 8), out=ops.person_flow_buffers(2, 9))
    out = ops.person_flow_buffers(2, 8)
    assert ops.person_flow(*mk(2, 8), out=out).rgb.data_ptr() == out.rgb.data_ptr()


def test_largest_scan_every_point_its_own_instance(ops):
    """N = 4096, the limit: eight chunks, all eight slots of every thread in use."""
    N = 4096
    rng = np.random.default_rng(9)
    inst = np.stack([rng.permutation(N) + 1, np.full(N, 4096)]).astype(np.int32)
    flow = rng.normal(0, 0.05, (2, N, 2)).astype(np.float32)
    out = ops.person_flow(_cuda(flow), ops.phi_table(np.radians(0.05), N), _cuda(inst), _cuda(np.array([N, N], np.int32)),
                          torch.zeros(2, N, 2, dtype=torch.float64, device="cuda"),
                          torch.zeros(2, N, dtype=torch.float64, device="cuda"))
    got = _host(out)
    assert np.array_equal(got["det_flow"][0][inst[0] - 1], got["flow_world"][0])
    assert np.array_equal(got["det_rgb"][0][inst[0] - 1], got["rgb"][0])
    want, count = sequential_means(inst[1], N, got["flow_world"][1])
    assert np.array_equal(got["det_flow"][1], want, equal_nan=True) and np.array_equal(got["det_count"][1], count)
    assert count[-1] == N


# ------------------------------------------------------------------ 5. streaming
class _DiffFlow(torch.nn.Module):
    """A deterministic elementwise 'flow net': (previous scan, scan) [B,N,1] -> [B,N,2]."""

    def forward(self, prev, cur):
        d = (cur - prev)[..., 0]
        return torch.stack((d, 0.5 * d), dim=-1)


def _stream_model(seed):
    from planar_optical_flow_amd.src.depracted.model.dr_spaam import SpatialDROW
    torch.manual_seed(seed)
    return SpatialDROW(num_scans=5, num_pts=56, alpha=0.5, window_size=11, pedestrian_only=True).cuda().eval()


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for k in x:
            assert np.array_equal(x[k], y[k], equal_nan=True), k


def test_streaming_tail_graph_equals_eager_equals_per_scan_function(u):
    from planar_optical_flow_amd.streaming import StreamingDetector
    model, flow_model = _stream_model(13), _DiffFlow()
    B, T = 2, 5
    scans = torch.from_numpy(synth.make_batch(seed=31, B=B, T=T).scans).cuda()            # [B, T, 450]
    rng = np.random.default_rng(5)
    poses = np.cumsum(rng.normal(0, 0.05, (T, B, 3)), axis=0) + np.array([60.0, 100.0, 0.4])
    mk = lambda graph: StreamingDetector(model, batch=B, graph=graph, nms_min_dist=0.5, flow_model=flow_model,
                                         cls_thresh=CLS_THRESH)
    eager, graphed = mk(False), mk(True)
    phi = u.get_laser_phi()

    def feed(t, first):
        ce, re_ = (v.clone() for v in eager(scans[:, t], pose=poses[t]))
        cg, rg = graphed(scans[:, t], pose=poses[t])
        assert torch.equal(ce, cg) and torch.equal(re_, rg)
        (de, ie), (dg, ig) = eager.detections(), graphed.detections()
        assert np.array_equal(ie, ig) and all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(de, dg))
        if first:
            for det in (eager, graphed):
                with pytest.raises(RuntimeError):
                    det.person_flow()
            return
        (pe, oe), (pg, og) = eager.person_flow(), graphed.person_flow()
        _same(pe, pg)
        for k in FIELDS:
            assert np.array_equal(getattr(oe, k).cpu().numpy(), getattr(og, k).cpu().numpy(), equal_nan=True), k
        flow = flow_model(scans[:, t - 1].unsqueeze(-1), scans[:, t].unsqueeze(-1))
        for b in range(B):
            want = u.person_flow(scans[b, t].cpu().numpy(), phi, torch.sigmoid(cg[b]).double().cpu().numpy(),
                                 rg[b].double().cpu().numpy(), flow[b].cpu().numpy(), poses[t, b], poses[t - 1, b])
            assert np.array_equal(ig[b], want["instance_mask"])
            assert np.array_equal(og.flow_world[b].cpu().numpy(), want["flow_world"])
            assert np.array_equal(og.rgb[b].cpu().numpy(), want["rgb"])
            assert np.array_equal(pg[b]["dets_cls"], want["dets_cls"][:, 0])
            for k in ("dets_xy_world", "person_flow", "person_rgb", "count", "valid"):
                assert np.array_equal(pg[b][k], want[k], equal_nan=True), (t, b, k)

    for t in range(T):
        feed(t, first=(t == 0))
    assert graphed._graph is not None and eager._graph is None
    eager.reset(), graphed.reset()
    feed(3, first=True)                                               # a new sequence: no predecessor again
    # without a pose everything stays in the scanner frame
    graphed(scans[:, 4])
    res, out = graphed.person_flow()
    flow = flow_model(scans[:, 3].unsqueeze(-1), scans[:, 4].unsqueeze(-1))
    want = u.person_flow(scans[0, 4].cpu().numpy(), phi, torch.sigmoid(graphed.pred_cls[0]).double().cpu().numpy(),
                         graphed.pred_reg[0].double().cpu().numpy(), flow[0].cpu().numpy())
    assert np.array_equal(res[0]["person_flow"], want["person_flow"], equal_nan=True)
    assert np.array_equal(res[0]["dets_xy_world"], want["dets_xy_world"])


def test_streaming_tail_with_a_fused_prototype_and_none_without_flow_model():
    from planar_optical_flow_amd.src.depracted.model.prototype import Prototype
    from planar_optical_flow_amd.streaming import StreamingDetector
    model = _stream_model(14)
    torch.manual_seed(3)
    proto = Prototype(in_channel=1, max_displacement=5).cuda().eval().fuse_for_inference()
    B, T = 2, 4
    scans = torch.from_numpy(synth.make_batch(seed=33, B=B, T=T).scans).cuda()
    poses = np.cumsum(np.random.default_rng(6).normal(0, 0.05, (T, B, 3)), axis=0)
    eager, graphed = (StreamingDetector(model, batch=B, graph=gr, nms_min_dist=0.5, flow_model=proto) for gr in (False, True))
    for t in range(T):
        eager(scans[:, t], pose=poses[t]), graphed(scans[:, t], pose=poses[t])
        if t:
            (pe, oe), (pg, og) = eager.person_flow(), graphed.person_flow()
            _same(pe, pg)
            for k in FIELDS:
                assert np.array_equal(getattr(oe, k).cpu().numpy(), getattr(og, k).cpu().numpy(), equal_nan=True), k
            assert np.isfinite(og.flow_world.cpu().numpy()).all()
    assert graphed._graph is not None
    # a detector without flow_model allocates none of the tail's buffers and refuses a pose
    plain = StreamingDetector(model, batch=B, nms_min_dist=0.5)
    plain(scans[:, 0]), plain(scans[:, 1])
    for name in ("_prev_scan", "_pf_out", "_pose_dev", "_pose_rot", "_pose_trans", "_pose_flow_trans"):
        assert not hasattr(plain, name), name
    assert plain._flow_model is None
    with pytest.raises(RuntimeError):
        plain.person_flow()
    with pytest.raises(ValueError):
        plain(scans[:, 2], pose=poses[2])
    with pytest.raises(ValueError):
        StreamingDetector(model, batch=B, flow_model=proto)           # the masks come from the NMS
