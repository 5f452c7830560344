"""Every accepted combination of the streaming detector's pose source, per-person tail and tracks (26), through the
public surface only: after every scan the eager and the replayed detector hold the same bits in every output and in
every accessor that is available, each accessor raises exactly until its scans-seen requirement is met (and always when
its feature is off), and after ``reset()`` the same sequence gives the same bits again -- ids from 1, pose from zero.
The refused combinations raise ``ValueError``."""
import numpy as np
import pytest
import torch

from test_person_motion import same_bits

pytestmark = pytest.mark.gpu

B, N, T, FED = 2, 450, 8, 5
KEYED = ("keyframe", "keyframe_map")
DEAD_RECKONS = ("flow", "scan_match") + KEYED

# (pose source, tail, tracks, nms): 8 without a tail, 10 with a flow model, 8 with person_motion
CASES = [(src, None, False, nms) for src in ("none", "scan_match") + KEYED for nms in (False, True)] \
    + [(src, "flow", tr, True) for src in ("given", "flow", "scan_match") + KEYED for tr in (False, True)] \
    + [(src, "motion", tr, True) for src in ("given", "scan_match") + KEYED for tr in (False, True)]


class DiffFlow(torch.nn.Module):
    """An elementwise stand-in for a flow net: the scan difference and half of it."""
    def forward(self, prev, cur):
        d = (cur - prev)[..., 0]
        return torch.stack((d, 0.5 * d), dim=-1)


@pytest.fixture(scope="module")
def model():
    from planar_optical_flow_amd.src.depracted.model.dr_spaam import SpatialDROW
    torch.manual_seed(13)
    return SpatialDROW(num_scans=5, num_pts=56, alpha=0.5, window_size=11, pedestrian_only=True).cuda().eval()


@pytest.fixture(scope="module")
def sequence():
    from planar_optical_flow_amd import synth
    scans = torch.from_numpy(synth.make_batch(seed=9, B=B, T=T).scans).cuda()          # [B, T, N]
    poses = np.cumsum(np.random.default_rng(4).normal(0, 0.05, (T, B, 3)), axis=0)
    return scans, poses


@pytest.fixture(scope="module")
def gate_score(model, sequence):
    """The median score of the sequence's detections.  The detector's ``cls_thresh=0.0`` makes every detection count, and
    the NMS gives every point to one, so a pose fit gated at that score would have no point left to vote; gated at the
    median, the points of about half of the detections vote and the rest are kept out."""
    from planar_optical_flow_amd.streaming import StreamingDetector
    det, scores = StreamingDetector(model, batch=B, num_pts=N, nms_min_dist=0.5), []
    for t in range(FED):
        det(sequence[0][:, t])
        scores += [conf for _, conf in det.detections()[0]]
    return float(np.median(np.concatenate(scores)))


def _settings(case, gate_score):
    src, tail, tracks, nms = case
    kw = dict(batch=B, num_pts=N, cls_thresh=0.0, nms_min_dist=0.5 if nms else None)
    if src in DEAD_RECKONS:
        kw["ego_motion"] = dict(cls_thresh=gate_score) if src == "flow" else dict(method=src, cls_thresh=gate_score)
    if tail == "flow":
        kw["flow_model"] = DiffFlow()
    if tail == "motion":
        kw["person_motion"] = dict()
    if tracks:
        kw["tracks"] = dict()
    return kw


def _available(case, seen):
    """Which accessors answer after `seen` scans of a sequence."""
    src, tail, tracks, _ = case
    return {"person_flow": tail == "flow" and seen >= 2,
            "person_motion": tail == "motion" and seen >= 1,
            "ego_motion": src in DEAD_RECKONS and seen >= (1 if src in KEYED else 2),
            "tracks": tracks and seen >= 2}


def _leaves(obj, path=""):
    """Every array, tensor and scalar in a nest of dicts, lists and (named) tuples: (path, Python type, host array)."""
    if isinstance(obj, dict):
        return [leaf for k in obj for leaf in _leaves(obj[k], "%s.%s" % (path, k))]
    if isinstance(obj, (list, tuple)):
        return [leaf for i, v in enumerate(obj) for leaf in _leaves(v, "%s[%d]" % (path, i))]
    if isinstance(obj, torch.Tensor):
        return [(path, "tensor", obj.detach().cpu().numpy().copy())]
    return [(path, type(obj).__name__, np.array(obj))]


def _snapshot(det, case, seen):
    snap = {"pred_cls": det.pred_cls, "pred_reg": det.pred_reg, "feat_fused": det.feat_fused, "template": det.template}
    if case[3]:
        snap["detections"] = det.detections()
    for name, there in _available(case, seen).items():
        if there:
            snap[name] = getattr(det, name)()
    return _leaves(snap)


def _same(a, b, where):
    assert [(p, t) for p, t, _ in a] == [(p, t) for p, t, _ in b], where
    for (p, _, x), (_, _, y) in zip(a, b):
        assert same_bits(x, y), (where, p)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s-%s-%s" % (c[0], c[1] or "notail", "tracks" if c[2] else "notracks",
                                                                      "nms" if c[3] else "nonms"))
def test_eager_graph_availability_and_reset(case, model, sequence, gate_score):
    from planar_optical_flow_amd.streaming import StreamingDetector
    src, tail, tracks, nms = case
    scans, poses = sequence
    eager = StreamingDetector(model, graph=False, **_settings(case, gate_score))
    graphed = StreamingDetector(model, graph=True, **_settings(case, gate_score))

    def one_pass():
        snaps, pairs, live, ok, first_ids = [], 0, 0, 0, None
        for t in range(FED):
            for det in (eager, graphed):
                for name, there in _available(case, t).items():
                    if not there:
                        with pytest.raises(RuntimeError):
                            getattr(det, name)()
                det(scans[:, t], **(dict(pose=poses[t]) if src == "given" else {}))
            e, g = _snapshot(eager, case, t + 1), _snapshot(graphed, case, t + 1)
            _same(e, g, (t, "eager against graph"))
            snaps.append(g)
            now = _available(case, t + 1)
            if now["person_motion"]:
                pairs += sum(int((d["prev"] >= 0).sum()) for d in graphed.person_motion()[0])
            if now["tracks"]:
                ids = [tr["id"] for sensor in graphed.tracks()[0] for tr in sensor]
                live += len(ids)
                if first_ids is None and ids:
                    first_ids = ids
            if now["ego_motion"]:
                fits = graphed.ego_motion()[0]
                ok += sum(f["ok"] for f in fits)
                if t == 0:                                     # a keyframe method: the first scan seeds, from the start pose
                    assert not any(f["ok"] for f in fits) and not any(f["pose"].any() for f in fits)
        return snaps, pairs, live, ok, first_ids

    first = one_pass()
    for det in (eager, graphed):
        det.reset()
    again = one_pass()
    for t, (a, b) in enumerate(zip(first[0], again[0])):
        _same(a, b, (t, "first pass against the pass after reset()"))
    assert first[1:] == again[1:]
    _, pairs, live, ok, first_ids = first
    print("%s: %d pairs, %d live tracks, %d ok fits over %d scans of %d sensors" % (case, pairs, live, ok, FED, B))
    if tail == "motion":
        assert pairs > 0
    if tracks:
        assert live > 0 and min(first_ids) == 1
    if src in DEAD_RECKONS:
        assert ok > 0


def test_refused_combinations(model, sequence):
    from planar_optical_flow_amd.streaming import StreamingDetector
    scans, poses = sequence
    mk = lambda **kw: StreamingDetector(model, batch=B, num_pts=N, **kw)
    for kw in (dict(ego_motion=dict()),                                            # method="flow" without a flow model
               dict(ego_motion=dict(method="flow"), nms_min_dist=0.5),
               dict(tracks=dict(), nms_min_dist=0.5),                              # nothing that feeds the tracks
               dict(person_motion=dict(), flow_model=DiffFlow(), nms_min_dist=0.5),
               dict(person_motion=dict()),                                         # no NMS masks
               dict(flow_model=DiffFlow())):
        with pytest.raises(ValueError):
            mk(**kw)
    for kw in (dict(ego_motion=dict(method="scan_match")),                         # dead-reckons its own pose
               dict(ego_motion=dict(method="keyframe"), nms_min_dist=0.5, person_motion=dict()),
               dict(ego_motion=dict(), nms_min_dist=0.5, flow_model=DiffFlow()),
               dict(), dict(nms_min_dist=0.5)):                                    # no per-person stage
        with pytest.raises(ValueError):
            mk(**kw)(scans[:, 0], pose=poses[0])
    for kw in (dict(), dict(nms_min_dist=0.5, flow_model=DiffFlow()), dict(nms_min_dist=0.5, person_motion=dict())):
        with pytest.raises(ValueError):
            mk(**kw).reset(pose=poses[0])
