"""Every accepted combination of the streaming detector's pose source, per-person tail and tracks (26), through the
public surface only: after every scan the eager and the replayed detector hold the same bits in every output and in
every accessor that is available, each accessor raises exactly until its scans-seen requirement is met (and always when
its feature is off), and after ``reset()`` the same sequence gives the same bits again -- ids from 1, pose from zero.
The refused combinations raise ``ValueError``.

GRID_CASES are 20 more rows run by the same test body, with the grid stages on (a 128 x 192 grid): ``grid_map`` alone
and with ``grid_scroll`` under the four pose sources that it accepts, ``grid_map`` + ``grid_match`` with and without
``grid_scroll`` under ``scan_match`` (the one source it accepts), each with the ``motion`` tail and tracks and once
without a tail.  After ``reset()`` the grid is empty and its origin and the scroll's offset are back where the
constructor put them.

MAP_CASES are 24 more rows, again run by the same test body, with the stages that read the map (N15-N17): ``grid_map`` +
``track_map`` behind the ``motion`` tail under the four pose sources and once behind a flow model with a pose per call
(the stage then starts with the second scan); ``grid_map`` + ``grid_cast`` and ``grid_map`` + ``grid_cast`` +
``novel_segments`` under the four pose sources, the cast once without the NMS, the segments also as the grid map's gate
(``gate_map=True``, which excludes the NMS); and every one of ``grid_scroll``, ``track_map``, ``grid_cast`` and
``novel_segments`` on at once under the four pose sources, once more with ``grid_match`` and once behind a flow model.
``grid_cast()`` and ``novel_segments()`` answer after one scan, ``track_map()`` after two; after ``reset()`` the evidence
is zero; a row with ``track_map`` gathers evidence in some slot and a row with ``grid_cast`` finds MAP points after the
first scan."""
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


# (pose source, tail, tracks, nms, grid stages): the grid stages with every pose source the constructor accepts for them
GRID_STAGES = ("grid_map", "grid_scroll", "grid_match")
GRID_CASES = [(src, tail, tail is not None, True, grid)
              for sources, grids in ((("given", "scan_match") + KEYED, (("grid_map",), ("grid_map", "grid_scroll"))),
                                     (("scan_match",), (("grid_map", "grid_match"), ("grid_map", "grid_scroll", "grid_match"))))
              for grid in grids for src in sources for tail in ("motion", None)]
GRID_SIZE = (128, 192)

# (pose source, tail, tracks, nms, stages): the stages that read the map.  "gate_map" in the stages is no stage: it makes
# the novelty segments the grid map's gate
MAP_STAGES = ("track_map", "grid_cast", "novel_segments")
GIVEN_AND_RECKONED = ("given", "scan_match") + KEYED
_CAST, _SEGS = ("grid_map", "grid_cast"), ("grid_map", "grid_cast", "novel_segments")
_ALL = ("grid_map", "grid_scroll", "track_map", "grid_cast", "novel_segments")
MAP_CASES = [(src, "motion", True, True, ("grid_map", "track_map")) for src in GIVEN_AND_RECKONED] \
    + [("given", "flow", True, True, ("grid_map", "track_map"))] \
    + [(src, None, False, True, _CAST) for src in GIVEN_AND_RECKONED] \
    + [("scan_match", None, False, False, _CAST)] \
    + [(src, None, False, True, _SEGS) for src in GIVEN_AND_RECKONED] \
    + [(src, None, False, False, _SEGS + ("gate_map",)) for src in GIVEN_AND_RECKONED] \
    + [(src, "motion", True, True, _ALL) for src in GIVEN_AND_RECKONED] \
    + [("scan_match", "motion", True, True, _ALL + ("grid_match",))] \
    + [("given", "flow", True, True, _ALL)]


def _grid_of(case):
    return case[4] if len(case) > 4 else ()


def _case_id(c):
    base = "%s-%s-%s-%s" % (c[0], c[1] or "notail", "tracks" if c[2] else "notracks", "nms" if c[3] else "nonms")
    return base + "".join("-" + g for g in _grid_of(c))


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
    src, tail, tracks, nms = case[:4]
    kw = dict(batch=B, num_pts=N, cls_thresh=0.0, nms_min_dist=0.5 if nms else None)
    if src in DEAD_RECKONS:
        kw["ego_motion"] = dict(cls_thresh=gate_score) if src == "flow" else dict(method=src, cls_thresh=gate_score)
    if tail == "flow":
        kw["flow_model"] = DiffFlow()
    if tail == "motion":
        kw["person_motion"] = dict()
    if tracks:
        kw["tracks"] = dict()
    for stage in _grid_of(case):
        if stage != "gate_map":
            kw[stage] = dict(size=GRID_SIZE) if stage == "grid_map" else dict()
    if "gate_map" in _grid_of(case):
        kw["novel_segments"] = dict(gate_map=True)
    if _grid_of(case):
        kw["cls_thresh"] = gate_score                          # at 0.0 every point is a person's: none would enter the map
    return kw


def _available(case, seen):
    """Which accessors answer after `seen` scans of a sequence."""
    src, tail, tracks, _ = case[:4]
    there = {"person_flow": tail == "flow" and seen >= 2,
             "person_motion": tail == "motion" and seen >= 1,
             "ego_motion": src in DEAD_RECKONS and seen >= (1 if src in KEYED else 2),
             "tracks": tracks and seen >= 2}
    there.update({stage: stage in _grid_of(case) and seen >= 1 for stage in GRID_STAGES})
    there.update({stage: stage in _grid_of(case) and seen >= (2 if stage == "track_map" else 1) for stage in MAP_STAGES})
    return there


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


def _grid_state(det, case):
    """Where the grid stands between two sequences: (grid, origin) and with grid_scroll (base, offset), on the host."""
    state = [t.cpu().numpy().copy() for t in det._gm_state]
    if "grid_scroll" in _grid_of(case):
        state += [det._gs_state.base.cpu().numpy().copy(), det._gs_state.offset.cpu().numpy().copy()]
    return state


@pytest.mark.parametrize("case", CASES + GRID_CASES + MAP_CASES, ids=_case_id)
def test_eager_graph_availability_and_reset(case, model, sequence, gate_score):
    from planar_optical_flow_amd.streaming import StreamingDetector
    src, tail, tracks, nms = case[:4]
    scans, poses = sequence
    eager = StreamingDetector(model, graph=False, **_settings(case, gate_score))
    graphed = StreamingDetector(model, graph=True, **_settings(case, gate_score))
    built = [_grid_state(det, case) for det in (eager, graphed)] if _grid_of(case) else None

    def one_pass():
        snaps, pairs, live, ok, first_ids, evidence, on_map = [], 0, 0, 0, None, 0, 0
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
            if now.get("track_map"):
                evidence += int((graphed.track_map()[2].ev_points > 0).sum())
            if now.get("grid_cast") and t > 0:
                on_map += int((graphed.grid_cast().point_class == 1).sum())
        return snaps, pairs, live, ok, first_ids, evidence, on_map

    first = one_pass()
    for det in (eager, graphed):
        det.reset()
    if _grid_of(case):
        # the grid is zeroed, its origin and the scroll's base and offset are back where the constructor put them
        for det, was in zip((eager, graphed), built):
            now = _grid_state(det, case)
            assert not now[0].any() and all(same_bits(a, b) for a, b in zip(now, was))
            if "grid_scroll" in _grid_of(case):
                assert not now[3].any()
            if "track_map" in _grid_of(case):
                assert len(det._tm_state) == 7 and not any(t.any() for t in det._tm_state)
        known = [leaf for path, _, leaf in first[0][-1] if path.startswith(".grid_map[0][0]")]
        assert len(known) == 1 and known[0].shape == (B,) + GRID_SIZE and (known[0] > 0).any() and (known[0] < 0).any()
    again = one_pass()
    for t, (a, b) in enumerate(zip(first[0], again[0])):
        _same(a, b, (t, "first pass against the pass after reset()"))
    assert first[1:] == again[1:]
    _, pairs, live, ok, first_ids, evidence, on_map = first
    print("%s: %d pairs, %d live tracks, %d ok fits, %d slots with evidence, %d MAP points over %d scans of %d sensors"
          % (case, pairs, live, ok, evidence, on_map, FED, B))
    if "track_map" in _grid_of(case):
        assert evidence > 0
    if "grid_cast" in _grid_of(case):
        assert on_map > 0
    if tail == "motion":
        assert pairs > 0
    if tracks:
        assert live > 0 and min(first_ids) == 1
    if src in DEAD_RECKONS:
        assert ok > 0


def test_the_collector_stays_out_of_the_capture(model, sequence):
    """A collection inside the capture could free a dropped detector with its captured graph: ``_capture`` collects first
    and holds the collector off until the capture has ended.  Nothing is provoked here: a stage only notes, each time it
    is launched, whether the stream is capturing and whether the collector is enabled."""
    import gc
    from planar_optical_flow_amd.streaming import StreamingDetector
    scans, poses = sequence
    det = StreamingDetector(model, batch=B, num_pts=N, nms_min_dist=0.5, person_motion=dict())
    noted, launch = [], det._stages[0].launch

    def noting(first):
        noted.append((torch.cuda.is_current_stream_capturing(), gc.isenabled()))
        launch(first)

    det._stages = (det._stages[0]._replace(launch=noting),) + det._stages[1:]
    assert gc.isenabled()
    for t in range(3):
        det(scans[:, t], pose=poses[t])
    assert det._graph is not None and gc.isenabled()
    assert (True, False) in noted and (True, True) not in noted and (False, False) not in noted, noted


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
    # the grid stages
    grid, match = dict(size=GRID_SIZE), dict(method="scan_match")
    for kw in (dict(grid_match=dict(), grid_map=grid, ego_motion=dict(method="keyframe"), nms_min_dist=0.5),
               dict(grid_match=dict(), grid_map=grid, ego_motion=dict(method="keyframe_map"), nms_min_dist=0.5),
               dict(grid_match=dict(), grid_map=grid, nms_min_dist=0.5),           # a pose per call is not corrected
               dict(grid_match=dict(), grid_map=grid, ego_motion=match, nms_min_dist=0.5, flow_model=DiffFlow()),
               dict(grid_match=dict(), grid_map=grid, ego_motion=dict(), nms_min_dist=0.5, flow_model=DiffFlow()),
               dict(grid_match=dict(), ego_motion=match),                          # no grid to match against
               dict(grid_scroll=dict(), ego_motion=match),                         # no grid to scroll
               dict(grid_scroll=dict(), nms_min_dist=0.5, person_motion=dict()),
               dict(grid_map=grid, ego_motion=dict(), nms_min_dist=0.5, flow_model=DiffFlow())):      # method "flow"
        with pytest.raises(ValueError):
            mk(**kw)
    with pytest.raises(ValueError):                            # a dead-reckoning detector with a grid takes no pose
        mk(grid_map=grid, grid_scroll=dict(), ego_motion=match)(scans[:, 0], pose=poses[0])
