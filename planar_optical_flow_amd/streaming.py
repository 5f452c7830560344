"""Streaming DR-SPAAM inference as one hipGraph replay per scan.

The reference's deployment mode is ``SpatialDROW.forward(x, testing=True, fea_template=...)``
(src/depracted/model/dr_spaam.py:243-262): every new scan is cut out, run through the first two trunk
blocks, fused with the running template by the attention gate and classified; the fused template is fed
back on the next call: ~30 kernel launches per scan.  ``StreamingDetector`` keeps the scan, the template and
the outputs in fixed device buffers, captures the steady-state step once and replays it, so the host thread
issues one graph launch per scan instead of thirty kernel launches.  Measured on MI355X
(tools/bench_stream.py): the replay takes 0.57-0.60 ms per scan at one sensor and 2.11 ms at eight; the eager
step is host-bound at one sensor and took 0.60 to 2.35 ms on different boxes.  Outputs are bit-identical to the eager step.
A model fused with ``embed="hip"`` has its gate embedding as one HIP node for the scan and the template, and may keep
float16 storage (float16 cutout and template).

Behind the trunk (cutout, model, NMS) a scan runs the stages its detector was built with, always in this order and on
one stream, so a capture stays one linear chain: the keyframe launch; the scan matcher and its pose launch; the
grid scroll; the scan-to-grid match; the grid refine; the flow net; the flow fit and its pose launch; the per-person flow; the person motion; the track
update; the grid cast; the novelty segments; the grid map; the map check of the tracks; the copy of the scan into the previous-scan buffer.  The detector holds them as one table, built once: the eager step, a
capture's warm-up and the captured region are each a loop over it, the warm-up puts back exactly the state the table names, and
``reset()`` clears exactly that ("The stage table").  The paragraphs below say what each stage is.
With a ``flow_model`` the step ends in the per-person flow (``ops.person_flow``): a flow net on the previous
and the current scan, then one launch that turns its output, the NMS masks and the sensor pose into one world-frame
flow vector and colour per detection -- still one replay per scan, nothing per point crosses to the host.
With ``ego_motion`` the pose is not an input any more: ``ops.ego_motion`` fits the sensor's motion to the flow of the
points that are not people, ``ops.pose_advance`` dead-reckons the pose on the device, and the per-person launch reads
the pose terms it wrote -- two more nodes in the same linear chain, no host copy.
With ``tracks`` the chain ends in ``ops.track_update``: the detections of the scan are associated with
persistent tracks on the device, so a person keeps one id from scan to scan and has a filtered velocity.
With ``ego_motion=dict(method="scan_match")`` the motion comes from the two scans alone (``ops.scan_match``, DESIGN 8,
N8): no flow net is needed for a pose, and with one the matched motion stands in front of the per-person launch.
With ``ego_motion=dict(method="keyframe")`` every scan is matched against a keyframe that stays fixed until the sensor
has left it (``ops.keyframe_match``): one launch that keeps the keyframe, its bookkeeping and the pose on
the device, so the pose of a sensor that stands still or works in one place does not walk away.
With ``ego_motion=dict(method="keyframe_map")`` the sensor keeps a ring of keyframes (``ops.keyframe_map_match``, DESIGN
8, N10): coming back to a stored keyframe switches to it instead of storing a new one, and the next match re-anchors
the pose there -- still one launch, every decision on the device.
With ``person_motion`` and no flow net the step ends in ``ops.person_motion``: per detection the
world-frame centroid of its own scan points, paired with the previous scan's centroids on the device; the difference
stands in for the per-person flow, and with ``tracks`` it feeds ``ops.track_update`` in the same chain.
With ``grid_map`` the chain also holds ``ops.grid_map_update``: every scan is entered at the step's
pose into an occupancy grid per sensor that stays on the device, and every scan point learns what its cell held before.
With ``grid_match`` (and ``method="scan_match"`` plus ``grid_map``) ``ops.grid_match`` stands directly behind the scan
matcher's pose launch: the scan is scored against the grid at whole-cell shifts and a few rotations
around the pose, in integers, and a pose that has lost a scan pair is put back before any later stage reads it and
before the scan is entered into the map.
With ``grid_refine`` (and ``method="scan_match"`` plus ``grid_map``) ``ops.grid_refine`` stands directly behind that
position: a Gauss-Newton fit of the scan's endpoints to the interpolated grid, every scan, that ties the
dead-reckoned pose to the map below the size of a cell.
With ``grid_scroll`` (and ``grid_map``) ``ops.grid_scroll`` stands behind the pose launch and in front of every stage
that reads cells: a sensor that comes near a border of its grid has the grid shifted by whole tiles so
that it stands on the middle tile again, origin included, on the device -- the map follows a sensor that travels.
With ``grid_store`` (and ``grid_scroll``) that launch is ``ops.grid_scroll_store``: the tiles that scroll
out are kept in a store per sensor and come back bit for bit when the sensor returns, so the map behind the window is
as large as the store and a return finds it.
With ``track_map`` (and ``tracks`` plus ``grid_map``) ``ops.track_map`` stands behind the grid map: what
the grid says about the detection a track was matched with is summed per track slot on the device, and every track has
a class -- free-standing, unsupported, background -- that an intermittent false positive on a static object cannot shed.
With ``grid_cast`` (and ``grid_map``) ``ops.grid_cast`` stands directly in front of the grid map: every
beam is walked through the grid as the scans before this one left it, and every point learns whether it lies on the
surface the map predicts, in front of it in space known to be empty, behind it, or where the map knows nothing.
With ``novel_segments`` (and ``grid_cast``) ``ops.novel_segments`` stands directly behind the grid cast:
the runs of points in front of the map's surface become detections in the layout of the NMS's, so a mover the net does
not report is a detection row all the same; with ``gate_map`` they gate the grid map, which then does not burn them in.
With ``merge_detections`` (and ``novel_segments``) ``ops.merge_detections`` stands directly behind the segments (DESIGN 8,
N18) and the cast, the segments and the merge move in front of the person stages: the segments the NMS's confident
detections do not already hold are appended to the NMS's rows, and the person motion, the tracks, the map check of the
tracks and (with ``gate_map``) the grid map read that one record -- a person the net scores low is tracked and not burned
in.  The order is then: the pose launch; the grid scroll; the scan-to-grid match; the grid refine; the grid cast; the novelty segments; the
merge; the person motion; the track update; the grid map; the map check of the tracks; the copy of the scan.
"""
import gc
from collections import namedtuple

import numpy as np
import torch

from . import ops

_DEFAULT_CUTOUT = dict(fixed=True, centered=True, window_width=1.0, window_depth=0.5, num_cutout_pts=56,
                       padding_val=29.99, area_mode=True)


_MATCHERS = {"scan_match": ops.scan_match, "keyframe": ops.keyframe_match, "keyframe_map": ops.keyframe_map_match}


def stage_defaults(arg, cls_thresh=0.5, method="flow"):
    """What the dict given as the constructor argument ``arg`` ("ego_motion" with its ``method``, "tracks",
    "person_motion", "grid_map", "grid_match", "grid_refine", "grid_scroll", "grid_store", "track_map", "grid_cast", "novel_segments", "merge_detections") may hold, with the defaults: the settings of the ``ops`` wrapper behind it, as its
    signature has them (``ops.stage_settings``), and -- stated here and nowhere else -- what the detector overrides or
    adds.  ``cls_thresh``: the detector's."""
    if arg == "ego_motion" and method == "flow":
        # the displacement of a canonical flow under the rigid model, robustly: of ops.ego_motion's settings the dict
        # holds these three, and the fit is re-weighted by default
        kw = ops.stage_settings(ops.ego_motion)
        return dict({k: kw[k] for k in ("huber_delta", "iters", "max_range")}, huber_delta=0.02, iters=4,
                    cls_thresh=cls_thresh)
    if arg == "ego_motion":
        # keys: the ring's size, which ops.keyframe_map_buffers takes
        return dict(ops.stage_settings(_MATCHERS[method]), cls_thresh=cls_thresh,
                    **(dict(keys=16) if method == "keyframe_map" else {}))
    if arg == "tracks":
        return dict(ops.stage_settings(ops.track_update), max_tracks=64)
    if arg == "track_map":
        return ops.stage_settings(ops.track_map)
    if arg == "novel_segments":
        # det_known takes the detector's cls_thresh: it is not a key of the dict; gate_map: whether the segments gate
        # the grid map of the same scan
        kw = ops.stage_settings(ops.novel_segments)
        del kw["cls_thresh"]
        return dict(kw, gate_map=False)
    if arg == "merge_detections":
        # who is confident is decided by the detector's cls_thresh: it is not a key of the dict; gate_map: whether the
        # merged record, not the NMS's, gates the grid map of the same scan
        kw = ops.stage_settings(ops.merge_detections)
        del kw["cls_thresh"]
        return dict(kw, gate_map=True)
    if arg == "grid_store":
        return dict(slots=64)                                  # the size of ops.grid_store_state, not a wrapper's keyword
    if arg in ("grid_scroll", "grid_cast"):
        kw = ops.stage_settings({"grid_scroll": ops.grid_scroll, "grid_cast": ops.grid_cast}[arg])
        del kw["res"]                                          # the grid's: a key of grid_map's dict
        return kw
    # person_motion, grid_map, grid_match and grid_refine always take the detector's cls_thresh: it is not a key of
    # their dicts
    kw = ops.stage_settings({"person_motion": ops.person_motion, "grid_map": ops.grid_map_update,
                             "grid_match": ops.grid_match, "grid_refine": ops.grid_refine}[arg])
    del kw["cls_thresh"]
    if arg in ("grid_match", "grid_refine"):
        del kw["res"]                                          # the grid's: a key of grid_map's dict
    return dict(kw, res=0.1, size=512) if arg == "grid_map" else kw


def stage_settings(arg, given, cls_thresh=0.5, method="flow"):
    """``stage_defaults`` overridden by the dict the argument ``arg`` was given; a key that is not among them raises."""
    defaults = stage_defaults(arg, cls_thresh, method)
    unknown = set(given) - set(defaults)
    if unknown:
        raise ValueError("unknown %s settings: %s" % (arg, sorted(unknown)))
    return dict(defaults, **given)


class StreamingDetector:
    """``det = StreamingDetector(model)``; ``pred_cls, pred_reg = det(scan)`` per incoming scan.

    model: an eval-mode ``SpatialDROW`` on the GPU (``fuse_for_inference()`` is applied unless the model is fused
    already; a model fused with ``storage=torch.float16, embed="hip"`` streams with a float16 cutout and a float16
    template, the outputs stay float32; float16 storage with the library embedding is refused).  scan: [N] or [B, N]
    ranges (B independent sensors advance in lock-step).  The returned tensors are the detector's fixed output
    buffers -- valid until the next call; ``.clone()`` to keep them.  ``feat_fused`` (the window similarities
    of the last step, input of the flow head) and ``template`` are attributes.  ``reset()`` forgets the
    template, as at the start of a sequence.  ``graph=False`` runs the same step eagerly (reference for
    tests and timing).  With ``nms_min_dist`` (one-logit models) the greedy centre NMS of
    ``utils.nms_predicted_center`` runs inside the same step and ``detections()`` returns its result.

    ``flow_model`` (needs ``nms_min_dist``): an eval-mode module mapping (previous scan [B,N,1], scan [B,N,1]) to a
    canonical flow [B,N,2], e.g. a fused ``Prototype``.  The detector keeps the previous scan and runs the flow
    model and ``ops.person_flow`` as the tail of the step; ``det(scan, pose=(x, y, phi))`` ([3] or [B,3], the
    sensor's world pose at this scan; none = scanner frame) supplies the frame, and ``person_flow()`` returns the
    per-person result from the second scan of a sequence on.  ``cls_thresh`` is the score from which a detection
    counts as valid.

    ``ego_motion`` (needs ``flow_model``): None, or a dict of ``huber_delta`` (0.02), ``iters`` (4), ``max_range``
    (20.0) and ``cls_thresh`` (the detector's) for ``ops.ego_motion``.  The detector then takes no pose: the flow
    model's output over the points outside this scan's confident detections gives the motion since the previous scan,
    a [B,3] pose state on the device is advanced by it (``reset(pose=...)`` sets it, zeros by default), and the
    per-person flow is in the frame of that dead-reckoned pose.  ``ego_motion()`` returns the fit and the pose.
    With ``method="scan_match"`` (default ``"flow"``) the dict holds the settings of ``ops.scan_match`` instead
    (``window``, ``gate``, ``max_gap``, ``huber_delta``, ``iters``, ``eps_theta``, ``eps_u``, ``min_pivot``,
    ``max_range``, ``cls_thresh``): the motion is matched between the previous scan and this one, every step starts
    from the previous step's motion (from rest after a failed pair), and ``flow_model`` may be None -- the detector
    then only dead-reckons; with ``nms_min_dist`` the points of this scan's confident detections do not vote.
    With ``method="keyframe"`` the dict holds those settings and ``key_dist`` (0.3), ``key_rot`` (0.3), ``min_share``
    (0.5) and ``max_misses`` (2) of ``ops.keyframe_match``: the scan is matched against the sensor's keyframe, the pose
    is the keyframe's composed with that one match, and the launch replaces the keyframe on the device.  It runs from
    the first scan of a sequence on (which becomes the keyframe; ``ego_motion()`` reports ok = False there), and
    ``flow_model`` may be None.
    With ``method="keyframe_map"`` the dict holds those settings and ``keys`` (16) and ``revisit`` (0.5) of
    ``ops.keyframe_map_match``: a ring of ``keys`` keyframes per sensor, and a sensor that returns to within ``revisit``
    times ``key_dist`` / ``key_rot`` of a stored keyframe switches to it, so the next match re-anchors the pose on it.

    ``tracks`` (needs ``flow_model`` or ``person_motion``): None, or a dict of ``max_tracks`` (64) and the settings of ``ops.track_update``
    (``gate``, ``q``, ``r_pos``, ``r_vel``, ``v0_var``, ``max_misses``, ``min_hits``).  The step then ends in the track
    update on the per-person result: ``tracks()`` returns the live tracks and the track id of every detection from the
    second scan of a sequence on, and ``reset()`` forgets them (ids restart at 1).

    ``person_motion`` (needs ``nms_min_dist`` or ``merge_detections``, excludes ``flow_model``): None, or a dict of ``reach`` (0.5),
    ``min_points`` (3) and ``max_range`` (20.0) of ``ops.person_motion``.  Every step, the first of a sequence included,
    then ends in that launch behind the pose launch: with ``method="scan_match"`` ``ops.pose_advance`` writes the pose
    terms it reads, with ``"keyframe"`` / ``"keyframe_map"`` the keyframe launch does, and without ``ego_motion``
    ``det(scan, pose=...)`` supplies the frame as with a flow model.  ``person_motion()`` returns the per-person result
    from the first scan on (the displacements are NaN there), ``tracks`` is accepted without a flow model and is fed by
    it, and ``reset()`` forgets the previous scan's centroids.

    ``grid_map`` (needs a pose: ``ego_motion`` with ``method="scan_match"``, ``"keyframe"`` or ``"keyframe_map"``, or no
    ``ego_motion`` and ``det(scan, pose=...)``; ``method="flow"`` is refused): None, or a dict of ``res`` (0.1 m per
    cell), ``size`` (512 cells; or (H, W); multiples of 64) and ``max_range``, ``tol``, ``hit``, ``miss``, ``lo``,
    ``hi``, ``free_thresh`` of ``ops.grid_map_update``.  Every step, the first of a sequence included, then enters the
    scan into an occupancy grid per sensor at the step's pose; with ``nms_min_dist`` the points of this scan's
    confident detections are not burned in and ``det_points`` / ``det_free`` say per detection how many of its points
    lie on cells seen free.  ``grid_map()`` returns the grid and the per-point outputs, and ``reset()`` empties the
    grid and puts the start pose in its middle.

    ``grid_match`` (needs ``grid_map`` and ``ego_motion=dict(method="scan_match")``; with ``"keyframe"``,
    ``"keyframe_map"``, a pose per call or a ``flow_model`` it is refused, not built): None, or a dict of ``reach`` (4
    cells), ``rotations`` (9), ``rot_step`` (0.01 rad), ``min_points`` (50), ``min_score`` (20), ``min_gain`` (8) and
    ``max_range`` of ``ops.grid_match``.  Every step, the first of a sequence included, then scores the scan against
    the sensor's grid around the dead-reckoned pose, directly behind the pose launch, and moves the pose and its terms
    when a shifted or turned candidate is clearly better: what a failed scan pair lost is put back before the person
    stages and the grid update read the pose.  ``grid_match()`` returns what was found; ``reset()`` needs nothing new
    (an empty grid scores 0 and moves nothing).

    ``grid_refine`` (needs ``grid_map`` and ``ego_motion=dict(method="scan_match")``, with or without ``grid_match``;
    with ``"keyframe"``, ``"keyframe_map"``, a pose per call or a ``flow_model`` it is refused, not built): None, or a
    dict of ``cap`` (32), ``iters`` (8), ``min_points`` (50), ``min_pivot`` (1e-6), ``max_shift`` (2.0 cells),
    ``max_turn`` (0.05 rad), ``eps_shift`` (1e-3 cells), ``eps_turn`` (1e-5 rad) and ``max_range`` of
    ``ops.grid_refine``.  Every step, the first of a sequence included, then fits the dead-reckoned pose to the
    sensor's grid below the size of a cell, directly behind ``grid_match``'s position and in front of every stage that
    reads the pose terms: the slow drift of a pose composed from scan pairs does not reach the map.
    ``grid_refine()`` returns the fit; ``reset()`` needs nothing new (an empty grid is not ok and moves nothing).

    ``grid_scroll`` (needs ``grid_map``; works with every way that argument gets its pose, ``det(scan, pose=...)``
    included): None, or a dict of ``margin`` (None: a quarter of the grid's shorter side in whole tiles of 64 cells) of
    ``ops.grid_scroll``.  Every step, the first of a sequence included, then looks where the sensor stands in its grid,
    directly behind the pose launch and in front of ``grid_match`` and every other stage that reads cells: within
    ``margin`` cells of a border the grid and its origin are shifted by whole tiles so that the sensor's tile is the
    middle one again, and what scrolls in is unknown.  ``grid_scroll()`` returns the shift; ``reset()`` puts the grid
    back around the start pose and clears the offset.

    ``grid_store`` (needs ``grid_scroll``): None, or a dict of ``slots`` (64, in [1, 1024]), the tiles of 64 x 64 cells
    (8 KiB each) kept per sensor behind the grid.  The scroll is then ``ops.grid_scroll_store``, in the same place: a
    tile that scrolls out and is not all unknown goes into the store -- free slots first, then the slot written longest
    ago -- and a tile that scrolls in comes back from it bit for bit, so a sensor that returns to a mapped place finds
    its map.  ``grid_store()`` returns the tiles restored, stored, evicted and dropped by the last step;
    ``grid_scroll()`` returns the shift as before; ``reset()`` empties the store.  The store is part of the stage's
    warm-up snapshot, so the first captured step holds a second copy of it (batch x slots x 8 KiB) while it warms up.

    ``track_map`` (needs ``tracks`` and ``grid_map``; works with ``person_motion`` and every ``method`` that argument
    accepts, and with ``flow_model`` plus ``det(scan, pose=...)``): None, or a dict of ``occ_thresh`` (17), ``free_pct``
    (50), ``occ_pct`` (50), ``min_points`` (20), ``min_scans`` (3), ``travel`` (0.5 m) and ``cap`` (4096) of
    ``ops.track_map``.  Every step on which the track update runs then ends, behind the grid map, in one launch that adds
    what the grid said about each track's detection -- its points, those on cells seen free, those on cells already
    occupied -- to the track's slot and classes the track: 3 background, 1 free-standing, 2 unsupported, 0 undecided.
    ``track_map()`` returns the classes and the evidence; ``reset()`` forgets the evidence.  A scroll of the grid needs
    nothing here: the evidence is world coordinates and counts, not cells.

    ``grid_cast`` (needs ``grid_map``; works with every source of a pose ``grid_map`` accepts, with ``grid_scroll`` and
    ``grid_match``, with and without ``nms_min_dist``): None, or a dict of ``max_range`` (20.0), ``tol`` (None: the
    grid's ``res``), ``occ_thresh`` (17) and ``free_thresh`` (16) of ``ops.grid_cast``.  Every scan, the first of a
    sequence included, then runs ``ops.grid_cast`` directly in front of the grid map, behind the scroll and the
    scan-to-grid match: each beam is walked through the grid as the scans before this one left it, and each point is
    MAP, NOVEL, THROUGH or UNKNOWN (on an empty map every beam runs to the grid's edge and every point is UNKNOWN).
    ``grid_cast()`` returns the predicted scan and the classes.  The stage keeps nothing: ``reset()`` has nothing of
    its own to forget.

    ``novel_segments`` (needs ``grid_cast``; with and without ``nms_min_dist``): None, or a dict of ``jump`` (0.3 m),
    ``max_skip`` (2), ``min_points`` (3) and ``max_width`` (1.0 m) of ``ops.novel_segments`` and ``gate_map`` (False).
    Every scan, the first of a sequence included, then runs ``ops.novel_segments`` directly behind the grid cast and in
    front of the grid map: the NOVEL points are grouped into segments, and the kept ones are detections in the layout
    of the NMS's results.  With ``nms_min_dist`` ``det_known`` says how many points of a segment the detector's own
    confident detections (``cls_thresh``) hold.  ``gate_map=True`` (only without ``nms_min_dist``: merging two gates is
    not built) makes the segments the grid map's gate, so what the stage found is not burned in.
    ``novel_segments()`` returns the record.  The stage keeps nothing: ``reset()`` has nothing of its own to forget.

    ``merge_detections`` (needs ``novel_segments``, and so ``grid_cast`` and ``grid_map``; with and without
    ``nms_min_dist``; with a ``flow_model`` it is refused, not built): None, or a dict of ``absorb_pct`` (50) of
    ``ops.merge_detections`` and ``gate_map`` (True).  Every scan, the first of a sequence included, then runs the grid
    cast, the segments and ``ops.merge_detections`` in front of the person stages: a segment is absorbed when at least
    ``absorb_pct`` per cent of its points belong to a detection of the NMS with a score >= ``cls_thresh``, the others are
    appended to the NMS's rows.  ``person_motion``, ``tracks`` and ``track_map`` read the merged record, and
    ``person_motion()``, ``tracks()`` and ``track_map()`` answer per merged row; ``detections()`` stays the NMS's.  With
    ``gate_map`` the grid map takes the merged record as its gate (``novel_segments=dict(gate_map=True)`` is refused
    beside it: one gate), without it the NMS's as before.  Without ``nms_min_dist`` the primary record is absent, every
    segment with a point is a row, and ``person_motion`` is accepted without ``nms_min_dist``: the chain needs no
    detector net.  ``merged_detections()`` returns the record.  The stage keeps nothing: ``reset()`` has nothing of its
    own to forget."""

    # One stage of a scan behind the trunk.  launch(first) enqueues it on the current stream (first: the first scan of a
    # sequence) and writes only fixed buffers; state: the tensors it advances, which a capture's warm-up puts back;
    # reset: forgets them at the start of a sequence; from_first: the first scan of a sequence runs it; warm_up: a
    # capture's warm-up runs it.
    _Stage = namedtuple("_Stage", "launch state reset from_first warm_up", defaults=((), None, True, True))

    def __init__(self, model, num_pts=450, batch=1, angle_inc=None, cutout_kwargs=None, graph=True, device="cuda",
                 nms_min_dist=None, flow_model=None, cls_thresh=0.5, ego_motion=None, tracks=None, person_motion=None,
                 grid_map=None, grid_match=None, grid_scroll=None, track_map=None, grid_cast=None,
                 novel_segments=None, merge_detections=None, grid_refine=None, grid_store=None):
        if not torch.cuda.is_available():
            raise RuntimeError("StreamingDetector needs the GPU (no CPU path)")
        self._refuse_float16(model)
        self.model = model.to(device).eval()
        # The captured graph bakes in the addresses of the folded trunk parameters (model._fused).  The detector
        # therefore (i) does not re-fuse a model that is already fused -- that would free the tensors another
        # detector's graph still replays from -- and (ii) keeps its own reference to the set it captured, so the
        # memory outlives a later fuse_for_inference() / train() of the model; _ensure_fused() notices such a
        # change before every step and drops the stale graph.
        if getattr(self.model, "_fused", None) is None:
            self.model.fuse_for_inference()
        self._fused_ref = self.model._fused
        self._route = self._fuse_route()
        self.kw = dict(_DEFAULT_CUTOUT if cutout_kwargs is None else cutout_kwargs)
        self.B, self.N = int(batch), int(num_pts)
        dev = next(self.model.parameters()).device
        self.tab = ops.phi_table(num_pts=self.N, device=dev) if angle_inc is None \
            else ops.phi_table(angle_inc, self.N, device=dev)
        self._scan = torch.zeros((self.B, 1, self.N), dtype=torch.float32, device=dev)
        # the cutout's per-sample workspace is the detector's, allocated before any capture: the captured step
        # then holds no allocation that is made and dropped inside the capture
        self._cut_ws = torch.zeros(max(self.B, 1), dtype=torch.int32, device=dev)
        self._use_graph = bool(graph)
        self._nms = None if nms_min_dist is None else float(nms_min_dist)
        self._dets = None
        self._graph = None
        self.template = None            # fixed buffer once the first scan has been seen
        self._seen = 0                  # scans since reset(), saturating at 2
        self.feat_fused = self.pred_cls = self.pred_reg = None
        # what a feature was built with, None without it; _filter_kw: the settings of ops.track_update (a detector
        # without tracks carries no data attribute named after them, tests/test_tracks_gpu.py holds it to that)
        self._flow_model = self._ego_kw = self._match_kw = self._key_kw = self._pm_kw = self._filter_kw = None
        self._gm_kw = self._sg_kw = self._gs_kw = self._tm_kw = self._gc_kw = self._ns_kw = self._mg_kw = None
        self._gr_kw = self._st_kw = None
        if person_motion is not None:
            if flow_model is not None:
                raise ValueError("person_motion stands in for the per-person flow: give flow_model or person_motion")
            if self._nms is None and merge_detections is None:
                raise ValueError("person_motion needs nms_min_dist: the centroids are taken over the NMS masks")
        method = "flow" if ego_motion is None else dict(ego_motion).get("method", "flow")
        if method not in ("flow", "scan_match", "keyframe", "keyframe_map"):
            raise ValueError("ego_motion method must be 'flow', 'scan_match', 'keyframe' or 'keyframe_map'")
        if ego_motion is not None and method == "flow" and flow_model is None:
            raise ValueError("ego_motion needs flow_model: the motion is fitted to the flow field "
                             "(method='scan_match' and method='keyframe' match the scans themselves)")
        if grid_map is not None and ego_motion is not None and method == "flow":
            raise ValueError("grid_map with ego_motion method='flow' is not built: use 'scan_match', 'keyframe' or "
                             "'keyframe_map', or no ego_motion and det(scan, pose=...)")
        if grid_match is not None:
            if grid_map is None or method != "scan_match" or ego_motion is None:
                raise ValueError("grid_match corrects the pose of ego_motion method='scan_match' against grid_map: with "
                                 "'keyframe', 'keyframe_map' or det(scan, pose=...) it is not built")
            if flow_model is not None:
                raise ValueError("grid_match with a flow_model is not built: flow_trans is not corrected")
        if grid_refine is not None:
            if grid_map is None or method != "scan_match" or ego_motion is None:
                raise ValueError("grid_refine fits the pose of ego_motion method='scan_match' to grid_map: with "
                                 "'keyframe', 'keyframe_map' or det(scan, pose=...) it is not built")
            if flow_model is not None:
                raise ValueError("grid_refine with a flow_model is not built: flow_trans is not corrected")
        if grid_scroll is not None and grid_map is None:
            raise ValueError("grid_scroll scrolls the grid of grid_map: give both")
        if grid_store is not None and grid_scroll is None:
            raise ValueError("grid_store keeps what grid_scroll moves out of the grid: give both")
        if grid_cast is not None and grid_map is None:
            raise ValueError("grid_cast walks the grid of grid_map: give both")
        if novel_segments is not None:
            if grid_cast is None or grid_map is None:
                raise ValueError("novel_segments groups the classes of grid_cast: give both (and grid_map)")
            if dict(novel_segments).get("gate_map") and self._nms is not None:
                raise ValueError("novel_segments gate_map with nms_min_dist is not built: the grid map takes one gate, "
                                 "and merging the segments with the NMS's rows is its own change")
        if merge_detections is not None:
            missing = [k for k, v in (("novel_segments", novel_segments), ("grid_cast", grid_cast),
                                      ("grid_map", grid_map)) if v is None]
            if missing:
                raise ValueError("merge_detections appends the rows of novel_segments, which groups the classes of "
                                 "grid_cast over grid_map: %s missing" % " and ".join(missing))
            if flow_model is not None:
                raise ValueError("merge_detections with a flow_model is not built: the per-person flow is aggregated "
                                 "over the NMS masks")
            if dict(novel_segments).get("gate_map"):
                raise ValueError("merge_detections with novel_segments gate_map: the grid map takes one gate -- "
                                 "merge_detections=dict(gate_map=True) gates it by the merged record, which holds the "
                                 "segments; drop novel_segments' gate_map")
        if track_map is not None and (tracks is None or grid_map is None):
            raise ValueError("track_map joins the tracks of tracks with the grid of grid_map: give both")
        self._cls_thresh = float(cls_thresh)
        if tracks is not None and flow_model is None and person_motion is None:
            raise ValueError("tracks needs flow_model: the tracks are fed by the per-person flow")
        if flow_model is not None and self._nms is None:
            raise ValueError("flow_model needs nms_min_dist: the per-person flow is aggregated over the NMS masks")
        ego = {k: v for k, v in (ego_motion or {}).items() if k != "method"}
        self._key_map = method == "keyframe_map"

        # Everything a stage touches is allocated here, before any capture, and the stages are listed in the order a
        # scan runs them.
        self._terms = ()                # (rot, trans, flow_trans) where a per-person stage reads them
        self._prev_pose = None
        if flow_model is not None or person_motion is not None or grid_map is not None:
            self._alloc_pose_terms(dev)
        keeps_scan = flow_model is not None or method == "scan_match"
        if keeps_scan:
            self._prev_scan = torch.zeros((self.B, self.N, 1), dtype=torch.float32, device=dev)
        Stage, stages = self._Stage, []
        if method == "keyframe" or self._key_map:
            kw = stage_settings("ego_motion", ego, self._cls_thresh, method)
            # the keyframe (or the ring of them), its bookkeeping and the pose live on the device
            if self._key_map:
                self._key_state = ops.keyframe_map_buffers(self.B, self.N, kw.pop("keys"), dev)
                self._key_out = ops.keyframe_map_match_buffers(self.B, self.N, dev)
                if not 0.0 <= float(kw["revisit"]) <= 1.0:
                    raise ValueError("revisit must be in [0, 1]")
                self._key_match, self._key_reset = ops.keyframe_map_match, ops.keyframe_map_reset
            else:
                self._key_state = ops.keyframe_buffers(self.B, self.N, dev)
                self._key_out = ops.keyframe_match_buffers(self.B, self.N, dev)
                self._key_match, self._key_reset = ops.keyframe_match, ops.keyframe_reset
            self._key_kw = kw
            self._key_terms = dict(zip(("rot", "trans", "flow_trans"), self._terms))
            self._pose_state = self._key_state.pose
            stages.append(Stage(self._keyframe_stage, tuple(self._key_state),
                                lambda: self._key_reset(self._key_state)))        # the next scan becomes the keyframe
        if method == "scan_match":
            self._match_kw = stage_settings("ego_motion", ego, self._cls_thresh, method)
            self._match_out = ops.scan_match_buffers(self.B, self.N, dev)     # its motion is also the next step's init
            self._pose_state = torch.zeros((self.B, 3), dtype=torch.float64, device=dev)
            from_first = person_motion is not None or grid_map is not None
            if from_first:
                # the first scan of a sequence has no pair to match: a pose launch without ok writes the pose terms
                self._pm_no_ok = torch.zeros(self.B, dtype=torch.uint8, device=dev)
            stages.append(Stage(self._match_stage, (self._match_out.motion, self._pose_state),
                                self._match_out.motion.zero_,                    # the first pair starts from rest
                                from_first=from_first))
        if grid_scroll is not None:
            # behind the pose launch (with a pose per call the terms are copied in before any stage) and in front of
            # every stage that reads cells: the search window of grid_match must not hang over a border.  The grid is
            # allocated below, so the stage reads self._gm_state when it runs; the grid and its origin are in the grid
            # stage's snapshot, base and offset in this one's
            self._gs_kw = stage_settings("grid_scroll", grid_scroll)
            shape = ops.grid_shape(stage_settings("grid_map", grid_map)["size"])
            ops.grid_scroll_margin(*shape, self._gs_kw["margin"])
            self._gs_state = ops.grid_scroll_state(self.B, *shape, dev)
            self._gs_out = ops.grid_scroll_buffers(self.B, dev)
            if grid_store is None:
                stages.append(Stage(self._grid_scroll_stage, (self._gs_state.base, self._gs_state.offset)))
            else:
                # the same entry of the table, the storing launch: the store's persistent fields join the snapshot
                self._st_kw = stage_settings("grid_store", grid_store)
                self._st_state = ops.grid_store_state(self.B, *shape, self._st_kw["slots"], dev)
                self._st_out = ops.grid_scroll_store_buffers(self.B, dev)
                self._gs_out = ops.GridScroll(self._st_out.shift, self._st_out.scrolled)
                stages.append(Stage(self._grid_scroll_stage, (self._gs_state.base, self._gs_state.offset) +
                                    tuple(getattr(self._st_state, k) for k in ops.GridStoreState.persistent)))
        if grid_match is not None:
            # directly behind the pose launch: every later stage reads the corrected terms.  The grid is allocated
            # below, so the stage reads self._gm_state when it runs; it advances nothing but the pose, which is in
            # the match stage's snapshot, and from an empty grid it is not ok
            kw = stage_settings("grid_match", grid_match)
            self._sg_out = ops.grid_match_buffers(self.B, kw["reach"], kw["rotations"], dev)
            self._sg_table = ops.grid_match_table(kw["rot_step"], kw["rotations"], dev)
            for k in ("min_points", "min_score", "min_gain"):
                if int(kw[k]) < 0:
                    raise ValueError("grid_match %s must be >= 0" % k)
            self._sg_kw = dict(kw, cls_thresh=self._cls_thresh)
            stages.append(Stage(self._grid_match_stage))
        if grid_refine is not None:
            # directly behind grid_match's position -- behind the pose launch and the scroll, and behind the whole-cell
            # search where that runs -- and in front of every stage that reads the pose terms.  Like grid_match it reads
            # self._gm_state when it runs and advances nothing but the pose, which is in the match stage's snapshot;
            # from an empty grid it is not ok
            kw = stage_settings("grid_refine", grid_refine)
            ops.grid_refine_check(kw["cap"], kw["iters"], kw["min_points"], min_pivot=kw["min_pivot"],
                              max_shift=kw["max_shift"], max_turn=kw["max_turn"])
            self._gr_out = ops.grid_refine_buffers(self.B, dev)
            self._gr_kw = dict(kw, cls_thresh=self._cls_thresh)
            stages.append(Stage(self._grid_refine_stage))
        def cast_stages():
            # the grid cast, the novelty segments and the merge: directly in front of the grid map, or with
            # merge_detections in front of the person stages, which then read the merged record; the grid is allocated
            # below and read when a stage runs
            if grid_cast is None:
                return
            # directly in front of the grid map, which it reads as the scans before this one left it, and behind the
            # scroll and the scan-to-grid match; it advances nothing
            kw = stage_settings("grid_cast", grid_cast)
            if not float(kw["max_range"]) > 0.0 or (kw["tol"] is not None and not float(kw["tol"]) >= 0.0) or \
                    int(kw["occ_thresh"]) < 1 or int(kw["free_thresh"]) < 0:
                raise ValueError("grid_cast: max_range must be > 0, tol >= 0 (or None), occ_thresh >= 1 and "
                                 "free_thresh >= 0")
            self._gc_kw = kw
            self._gc_out = ops.grid_cast_buffers(self.B, self.N, dev)
            stages.append(Stage(self._grid_cast_stage))
            if novel_segments is not None:
                # directly behind the cast, whose classes it groups, and in front of the grid map, which it may gate;
                # it advances nothing
                kw = stage_settings("novel_segments", novel_segments)
                if not float(kw["jump"]) > 0.0 or not float(kw["max_width"]) >= 0.0 or int(kw["min_points"]) < 1 or \
                        not 0 <= int(kw["max_skip"]) <= 64:
                    raise ValueError("novel_segments: jump must be > 0, max_width >= 0, min_points >= 1 and "
                                     "max_skip in [0, 64]")
                self._ns_gates = bool(kw.pop("gate_map"))
                self._ns_kw = dict(kw, cls_thresh=self._cls_thresh)
                self._ns_out = ops.novel_segments_buffers(self.B, self.N, dev)
                stages.append(Stage(self._novel_segments_stage))
            if merge_detections is not None:
                # directly behind the segments, whose rows it appends to the NMS's; it advances nothing
                kw = stage_settings("merge_detections", merge_detections)
                if not 0 <= int(kw["absorb_pct"]) <= 101:
                    raise ValueError("merge_detections: absorb_pct must be in [0, 101]")
                self._mg_gates = bool(kw.pop("gate_map"))
                self._mg_kw = dict(kw, cls_thresh=self._cls_thresh)
                self._mg_out = ops.merge_detections_buffers(self.B, self.N, dev)
                stages.append(Stage(self._merge_stage))

        if merge_detections is not None:
            cast_stages()
        if flow_model is not None:
            self._flow_model = flow_model.to(dev).eval()
            self._pf_out = ops.person_flow_buffers(self.B, self.N, dev)
            if ego_motion is not None and method == "flow":
                self._ego_kw = stage_settings("ego_motion", ego, self._cls_thresh, method)
                self._ego_out = ops.ego_motion_buffers(self.B, self.N, dev)
                self._pose_state = torch.zeros((self.B, 3), dtype=torch.float64, device=dev)
            stages.append(Stage(self._flow_stage, () if self._ego_kw is None else (self._pose_state,),
                                from_first=False))
        if person_motion is not None:
            kw = stage_settings("person_motion", person_motion)
            if not float(kw["reach"]) >= 0.0 or int(kw["min_points"]) < 1:
                raise ValueError("reach must be >= 0 and min_points >= 1")
            self._pm_kw = dict(kw, cls_thresh=self._cls_thresh)
            self._pm_out = ops.person_motion_buffers(self.B, self.N, dev)
            self._pm_state = ops.person_motion_state(self.B, self.N, dev)
            stages.append(Stage(self._motion_stage, tuple(self._pm_state),
                                lambda: ops.person_motion_reset(self._pm_state)))  # the next scan seeds the centroids
        if tracks is not None:
            kw = stage_settings("tracks", tracks)
            self._track_state = ops.track_buffers(self.B, kw.pop("max_tracks"), self.N, dev)
            self._filter_kw = kw
            stages.append(Stage(self._track_stage, tuple(self._track_state),
                                lambda: ops.track_reset(self._track_state), from_first=person_motion is not None))
        if grid_map is not None:
            kw = stage_settings("grid_map", grid_map)
            shape = ops.grid_shape(kw.pop("size"))
            if not float(kw["res"]) > 0.0:
                raise ValueError("grid_map res must be > 0")
            self._gm_kw = dict(kw, cls_thresh=self._cls_thresh)
            self._gm_state = ops.grid_map_state(self.B, *shape, dev)
            self._gm_out = ops.grid_map_buffers(self.B, self.N, dev)
            self._gm_centre(np.zeros((self.B, 2)))
            if merge_detections is None:
                cast_stages()
            stages.append(Stage(self._grid_stage, tuple(self._gm_state), self._gm_state.grid.zero_))
        if track_map is not None:
            # behind the track update and the grid map, whose outputs of this step it joins; it runs when the track
            # stage runs
            kw = stage_settings("track_map", track_map)
            if not self.N <= int(kw["cap"]) <= 1 << 20 or not float(kw["travel"]) >= 0.0 or \
                    any(not 0 <= int(kw[k]) <= 100 for k in ("free_pct", "occ_pct")) or \
                    any(int(kw[k]) < 0 for k in ("occ_thresh", "min_points", "min_scans")):
                raise ValueError("track_map: cap must be in [num_pts, 2^20], free_pct and occ_pct in [0, 100], travel, "
                                 "occ_thresh, min_points and min_scans >= 0")
            self._tm_kw = kw
            self._tm_state = ops.track_map_state(self.B, self._track_state.track_id.shape[1], dev)
            self._tm_out = ops.track_map_buffers(self.B, self._track_state.track_id.shape[1], self.N, dev)
            stages.append(Stage(self._track_map_stage, tuple(self._tm_state),
                                lambda: ops.track_map_reset(self._tm_state), from_first=person_motion is not None))
        if keeps_scan:
            # not in a warm-up: the captured step behind it reads the scan before this one
            stages.append(Stage(self._keep_scan, warm_up=False))
        self._stages = tuple(stages)

    def _alloc_pose_terms(self, dev):
        # trans | flow_trans | rot of every sensor in one buffer: one small copy per scan from a pinned staging
        # buffer allocated once (an event keeps the host from refilling it while its last copy is in flight)
        self._pose_dev = torch.zeros(self.B * 48, dtype=torch.uint8, device=dev)
        self._pose_trans, self._pose_flow_trans, self._pose_rot = self._pose_views(self._pose_dev)
        self._terms = (self._pose_rot, self._pose_trans, self._pose_flow_trans)
        self._pose_host = torch.zeros(self.B * 48, dtype=torch.uint8).pin_memory()
        self._pose_host_np = tuple(v.numpy() for v in self._pose_views(self._pose_host))
        self._pose_copied = torch.cuda.Event()

    @staticmethod
    def _refuse_float16(model):
        """Float16 storage streams only with the HIP embedding (fuse_for_inference(storage=float16, embed="hip")):
        the library embedding needs float32 rows, i.e. a widened copy of the scan's features and of the template per
        step."""
        if getattr(model, "_fused", None) is not None and getattr(model, "_storage", torch.float32) != torch.float32 \
                and getattr(model, "_embed_route", "library") != "hip":
            raise ValueError("StreamingDetector keeps float32 storage: the model was fused with storage=%s -- "
                             "call model.fuse_for_inference() (float32) first" % model._storage)

    def _fuse_route(self):
        return (getattr(self.model, "_storage", torch.float32), getattr(self.model, "_embed_route", "library"))

    def reset(self, pose=None):
        """Forget the template (and the previous scan).  pose ([3] or [B,3], ego-motion detectors only): the pose the
        dead reckoning starts from; zeros by default."""
        if pose is not None and not self._dead_reckons():
            raise ValueError("reset(pose=...) is only used with ego_motion")
        self._seen = 0
        self._prev_pose = None
        for stage in self._stages:
            if stage.reset is not None:
                stage.reset()
        if self._dead_reckons():
            start = np.zeros((self.B, 3)) if pose is None else np.broadcast_to(
                np.asarray(pose.detach().cpu().numpy() if isinstance(pose, torch.Tensor) else pose,
                           dtype=np.float64).reshape(-1, 3), (self.B, 3)).copy()
            self._pose_state.copy_(torch.from_numpy(start))
        if self._gm_kw is not None:
            # a detector that is given its pose centres the grid again on the first pose of the sequence (_set_pose)
            self._gm_centre(start[:, :2] if self._dead_reckons() else np.zeros((self.B, 2)))

    def _has_tracks(self):
        return self._filter_kw is not None

    def _dead_reckons(self):
        return self._ego_kw is not None or self._match_kw is not None or self._key_kw is not None

    def _ensure_fused(self):
        """The model was re-fused (new checkpoint) or left eval mode since the last step: fuse again if needed
        and forget the graph captured on the old parameter tensors."""
        if self.model.training:
            self.model.eval()
        if getattr(self.model, "_fused", None) is None:
            self.model.fuse_for_inference()
        self._refuse_float16(self.model)
        if self.model._fused is not self._fused_ref or self._fuse_route() != self._route:
            if self._fuse_route()[0] != self._route[0] and self.template is not None:
                # another storage type: the running template goes on in that type (a new buffer; the graph is dropped)
                self.template = self.template.to(self._fuse_route()[0])
            self._fused_ref = self.model._fused
            self._route = self._fuse_route()
            self._graph = None

    # one step on the static buffers; `first` = no template yet
    def _step(self, first):
        x = ops.cutout(self._scan, self.tab, workspace=self._cut_ws, out_dtype=self._route[0], **self.kw)
        with torch.no_grad():
            cls, reg, tmpl, fused = self.model(x, testing=True, fea_template=None if first else self.template)
            if self._nms is not None:
                if cls.shape[-1] != 1:
                    raise ValueError("nms_min_dist needs a one-logit (pedestrian_only) model")
                conf = torch.sigmoid(cls[..., 0]).double().contiguous()
                self._dets = ops.nms_predicted_center(self._scan[:, 0], self.tab, conf, reg.double().contiguous(), self._nms)
        return cls, reg, tmpl, fused

    def _person_dets(self):
        """The detection record the person stages read, in the order of ``_dets`` (xy, scores, counts, masks): the merged
        one with merge_detections, else the NMS's."""
        if self._mg_kw is None:
            return self._dets
        o = self._mg_out
        return o.det_xy, o.det_cls, o.num_det, o.instance_mask

    def _match_gate(self):
        """With the NMS the points of this scan's confident detections do not vote in a scan match."""
        if self._dets is None:
            return {}
        _, conf, num, inst = self._dets
        return dict(instance_mask=inst, num_det=num, det_cls=conf)

    # The keyframe launch runs on every scan, the first of a sequence included (it seeds there); in front of a
    # per-person stage it writes the pose terms that stage reads.
    def _keyframe_stage(self, first):
        self._key_match(self._scan[:, 0], self.tab, self._key_state, out=self._key_out, **self._match_gate(),
                        **self._key_terms, **self._key_kw)

    # The motion from the two scans alone, started from the previous step's (a NaN row, a failed pair, counts as zeros
    # in the kernel), then the pose and, in front of a per-person stage, the pose terms.  The first scan of a sequence
    # has no pair: in front of person_motion a pose launch without ok writes the pose terms.
    def _match_stage(self, first):
        if first:
            ops.pose_advance(self._match_out.motion, self._pm_no_ok, self._pose_state, *self._terms)
        else:
            m = ops.scan_match(self._prev_scan.view(self.B, self.N), self._scan[:, 0], self.tab,
                               init=self._match_out.motion, out=self._match_out, **self._match_gate(), **self._match_kw)
            ops.pose_advance(m.motion, m.ok, self._pose_state, *self._terms)

    # The flow net on (previous, current) scan; with method="flow" the sensor's motion from the flow outside this scan's
    # confident detections, then the pose launch, which writes the pose terms; then the per-person launch, which reads
    # them.
    def _flow_stage(self, first):
        xy, conf, num, inst = self._dets
        with torch.no_grad():
            flow = self._flow_model(self._prev_scan, self._scan.view(self.B, self.N, 1)).float().contiguous()
            if self._ego_kw is not None:
                ego = ops.ego_motion(self._scan[:, 0], self.tab, flow, instance_mask=inst, num_det=num, det_cls=conf,
                                     out=self._ego_out, **self._ego_kw)
                ops.pose_advance(ego.motion, ego.ok, self._pose_state, *self._terms)
            ops.person_flow(flow, self.tab, inst, num, xy, conf, *self._terms, self._cls_thresh, out=self._pf_out)

    # Behind the pose launch, on every scan of a sequence (the first one seeds).
    def _motion_stage(self, first):
        xy, conf, num, inst = self._person_dets()
        ops.person_motion(self._scan[:, 0], self.tab, inst, num, xy, conf, self._pose_rot, self._pose_trans,
                          self._pm_state, out=self._pm_out, **self._pm_kw)

    # On the result of whichever per-person stage the detector has.
    def _track_stage(self, first):
        o, (_, _, num, inst) = self._pf_out if self._pm_kw is None else self._pm_out, self._person_dets()
        ops.track_update(o.det_xy_world, o.det_flow, o.det_valid, num, inst, self._track_state, **self._filter_kw)

    # Behind the pose launch, on every scan of a sequence: the scan into the grid at this step's pose.
    def _grid_stage(self, first):
        gate = self._match_gate()
        if self._ns_kw is not None and self._ns_gates:         # the novelty segments of this scan are not burned in
            o = self._ns_out
            gate = dict(instance_mask=o.instance_mask, num_det=o.num_det, det_cls=o.det_cls)
        if self._mg_kw is not None and self._mg_gates:         # nor is what the merge appended to the NMS's rows
            o = self._mg_out
            gate = dict(instance_mask=o.instance_mask, num_det=o.num_det, det_cls=o.det_cls)
        ops.grid_map_update(self._scan[:, 0], self.tab, self._pose_rot, self._pose_trans, self._gm_state,
                            out=self._gm_out, **gate, **self._gm_kw)

    # Directly in front of the grid map, on every scan of a sequence: the scan the grid predicts, before this scan enters it.
    def _grid_cast_stage(self, first):
        ops.grid_cast(self._scan[:, 0], self.tab, self._pose_rot, self._pose_trans, self._gm_state,
                      res=self._gm_kw["res"], out=self._gc_out, **self._match_gate(), **self._gc_kw)

    # Directly behind the grid cast, on every scan of a sequence: its NOVEL points as detections.
    def _novel_segments_stage(self, first):
        ops.novel_segments(self._scan[:, 0], self.tab, self._gc_out.point_class, out=self._ns_out,
                           **self._match_gate(), **self._ns_kw)

    # Directly behind the novelty segments, on every scan of a sequence: their rows appended to the NMS's; without
    # nms_min_dist there are none of those and the primary record is absent.
    def _merge_stage(self, first):
        gate = self._match_gate()
        if gate:
            gate["det_xy"] = self._dets[0]
        ops.merge_detections(*self._ns_out[:4], out=self._mg_out, **gate, **self._mg_kw)

    # Behind the track update and the grid map of this step: the grid's word on every track's detection, per slot.
    def _track_map_stage(self, first):
        _, _, num, inst = self._person_dets()
        ops.track_map(self._track_state, self._gm_out, inst, num, self._tm_state, out=self._tm_out, **self._tm_kw)

    # Behind the scan matcher's pose launch and in front of everything that reads the pose terms: the pose against the
    # grid as the scans before this one left it.
    def _grid_match_stage(self, first):
        ops.grid_match(self._scan[:, 0], self.tab, self._pose_rot, self._pose_trans, self._pose_state, self._gm_state,
                       res=self._gm_kw["res"], table=self._sg_table, out=self._sg_out, **self._match_gate(),
                       **self._sg_kw)

    # Behind grid_match's position and in front of everything that reads the pose terms: the pose fitted to the grid as
    # the scans before this one left it, below the size of a cell.
    def _grid_refine_stage(self, first):
        ops.grid_refine(self._scan[:, 0], self.tab, self._pose_rot, self._pose_trans, self._pose_state, self._gm_state,
                        res=self._gm_kw["res"], out=self._gr_out, **self._match_gate(), **self._gr_kw)

    # Behind the pose launch and in front of every stage that reads cells: the grid follows the sensor.
    def _grid_scroll_stage(self, first):
        if self._st_kw is not None:
            ops.grid_scroll_store(self._pose_trans, self._gm_state, self._gs_state, self._st_state,
                                  res=self._gm_kw["res"], out=self._st_out, **self._gs_kw)
            return
        ops.grid_scroll(self._pose_trans, self._gm_state, self._gs_state, res=self._gm_kw["res"], out=self._gs_out,
                        **self._gs_kw)

    def _gm_centre(self, xy):
        """The origin that puts the world positions xy [B,2] in the middle of their grids (with grid_scroll: where the
        scrolling starts from)."""
        H, W = self._gm_state.grid.shape[1:]
        origin = np.asarray(xy, dtype=np.float64) - 0.5 * float(self._gm_kw["res"]) * np.array([W, H], dtype=np.float64)
        self._gm_state.origin.copy_(torch.from_numpy(origin))
        if self._gs_kw is not None:
            ops.grid_scroll_reset(self._gs_state, self._gm_state)
        if self._st_kw is not None:
            ops.grid_store_reset(self._st_state)

    def _keep_scan(self, first):
        self._prev_scan.copy_(self._scan.view(self.B, self.N, 1))

    def _pose_views(self, buf):
        nb = self.B
        return (buf[:16 * nb].view(torch.float64).view(nb, 2), buf[16 * nb:32 * nb].view(torch.float64).view(nb, 2),
                buf[32 * nb:].view(torch.float32).view(nb, 2, 2))

    def _set_pose(self, pose):
        """Pose terms of this scan, formed on the host as utils.person_flow forms them, into the fixed device buffers."""
        from .src.utils.utils import _pose_terms
        cur = None
        if pose is not None:
            cur = np.asarray(pose.detach().cpu().numpy() if isinstance(pose, torch.Tensor) else pose, dtype=np.float64)
            cur = np.broadcast_to(cur.reshape(-1, 3), (self.B, 3)).copy()
        terms = _pose_terms(cur, self._prev_pose if cur is not None else None, batch=self.B)
        self._prev_pose = cur
        if self._gm_kw is not None and self._seen == 0:
            self._gm_centre(np.zeros((self.B, 2)) if cur is None else cur[:, :2])
        self._pose_copied.synchronize()               # the staging buffer's previous copy has left it
        for dst, src in zip(self._pose_host_np, (terms[1], terms[2], terms[0])):
            dst[...] = src
        self._pose_dev.copy_(self._pose_host, non_blocking=True)
        self._pose_copied.record()

    def _store_template(self, tmpl):
        if self.template is None:
            self.template = tmpl.clone()              # allocated once: the captured graph holds its address
        else:
            self.template.copy_(tmpl)

    def _capture(self):
        side = torch.cuda.Stream(device=self._scan.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                 # warm-up off the capture: library handles, lazy inits
            # it reads the template and the previous scan and writes the output buffers; what it advances besides --
            # pose, match move, keyframe, centroids, tracks (ids and ages would run ahead) -- is put back
            state = [t for stage in self._stages for t in stage.state]
            saved = [t.clone() for t in state]
            for _ in range(2):
                self._step(False)
                for stage in self._stages:
                    if stage.warm_up:
                        stage.launch(False)
            for t, was in zip(state, saved):
                t.copy_(was)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        # A detector that was dropped is held by cycles (its stages are bound methods) until Python's collector runs,
        # and with it its captured graph and the graph's memory pool.  A collection that starts inside the capture
        # would destroy them there, which a capture in progress does not survive: collect now and keep the collector
        # off until the capture has ended.
        gc.collect()
        collecting = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(g):
                cls, reg, tmpl, fused = self._step(False)
                self.template.copy_(tmpl)             # feed the fused template back in place
                for stage in self._stages:
                    stage.launch(False)
        finally:
            if collecting:
                gc.enable()
        self._graph, self._out, self._graph_dets = g, (cls, reg, fused), self._dets

    def __call__(self, scan, pose=None):
        scan = torch.as_tensor(scan, dtype=torch.float32)
        self._ensure_fused()
        if self._dead_reckons():
            if pose is not None:
                raise ValueError("an ego_motion detector takes no pose: it dead-reckons its own (reset(pose=...))")
        elif self._flow_model is not None or self._pm_kw is not None or self._gm_kw is not None:
            self._set_pose(pose)
        elif pose is not None:
            raise ValueError("pose is only used with a flow_model")
        self._scan.copy_(scan.reshape(self.B, 1, self.N), non_blocking=True)
        first = self._seen == 0                       # first scan of a sequence: eager, template = its own features
        if first or not self._use_graph:
            cls, reg, tmpl, fused = self._step(first)
            self._store_template(tmpl)
            for stage in self._stages:
                if stage.from_first or not first:
                    stage.launch(first)
        else:
            if self._graph is None:
                self._capture()                       # warm-up steps read the template, nothing writes it
            self._graph.replay()                      # the captured step holds the stages itself
            cls, reg, fused = self._out
            self._dets = self._graph_dets
        self._seen = min(self._seen + 1, 2)
        self.pred_cls, self.pred_reg, self.feat_fused = cls, reg, fused
        return cls, reg

    def detections(self):
        """-> list (one entry per sensor) of (xy [M, 2], confidence [M]) NumPy arrays and the instance masks [B, N]
        of the last step (needs ``nms_min_dist``).  Reads the counts back, i.e. synchronises."""
        if self._dets is None:
            raise RuntimeError("construct the detector with nms_min_dist and feed it a scan first")
        xy, conf, num, inst = self._dets
        counts = num.cpu().numpy()
        return [(xy[b, :m].cpu().numpy(), conf[b, :m].cpu().numpy()) for b, m in enumerate(counts)], inst.cpu().numpy()

    def _per_detection(self, o, **fields):
        """One dict per sensor of the rows of its detections: the scores, and under every key the field of ``o`` it
        names."""
        _, conf, num, _ = self._person_dets()
        host = lambda t, b, m: t[b, :m].cpu().numpy()
        return [dict({k: host(getattr(o, f), b, m) for k, f in fields.items()}, dets_cls=host(conf, b, m),
                     valid=host(o.det_valid, b, m).astype(bool)) for b, m in enumerate(num.cpu().numpy())]

    def person_flow(self):
        """-> list (one dict per sensor) of the last step's per-person result, as ``utils.person_flow`` returns it
        without the per-point entries: dets_xy_world [M,2], dets_cls [M], person_flow [M,2], person_rgb [M,3],
        count [M], valid [M]; and the device-resident per-point outputs (``ops.PersonFlow``, valid until the next
        call).  Needs ``flow_model`` and two scans of a sequence: the first one has no predecessor (the reference
        skips that frame too).  Reads the counts back, i.e. synchronises."""
        if self._flow_model is None or self._seen < 2:
            raise RuntimeError("construct the detector with flow_model and feed it two scans of a sequence first")
        return self._per_detection(self._pf_out, dets_xy_world="det_xy_world", person_flow="det_flow",
                                   person_rgb="det_rgb", count="det_count"), self._pf_out

    def person_motion(self):
        """-> list (one dict per sensor) of the last step's per-person result, with the per-detection keys of
        ``person_flow()`` -- dets_xy_world [M,2], dets_cls [M], person_flow [M,2] (the displacement since the previous
        scan; NaN without a partner, so on the first scan of a sequence), count [M], valid [M] -- and centre [M,2], prev
        [M] (the partner's row in the previous scan or -1); and the device-resident outputs (``ops.PersonMotion``, valid
        until the next call).  Needs ``person_motion`` and one scan.  Reads the counts back, i.e. synchronises."""
        if self._pm_kw is None or self._seen < 1:
            raise RuntimeError("construct the detector with person_motion and feed it a scan first")
        return self._per_detection(self._pm_out, dets_xy_world="det_xy_world", person_flow="det_flow", count="det_count",
                                   centre="det_centre", prev="det_prev"), self._pm_out

    def grid_map(self):
        """-> (the device-resident ``ops.GridMapState``: grid [B,H,W] int16 log-odds counts and origin [B,2];  the
        last step's ``ops.GridMapOut``: point_cell, point_mark, point_prior [B,N] and det_points, det_free [B,N] in
        the row order of ``detections()``, valid until the next call).  Needs ``grid_map`` and one scan.  No
        synchronisation: the tensors stay on the device."""
        if self._gm_kw is None or self._seen < 1:
            raise RuntimeError("construct the detector with grid_map and feed it a scan first")
        return self._gm_state, self._gm_out

    def grid_match(self):
        """-> (list with one dict per sensor of the last step's scan-to-grid match: best [3] = (rotation steps, dy, dx
        in cells), score [2] = (the best candidate's, the incoming pose's), votes, ok, moved and correction [3] = what
        was added to (x, y, phi);  the device-resident ``ops.GridMatch``, valid until the next call).  Needs
        ``grid_match`` and one scan.  Synchronises."""
        if self._sg_kw is None or self._seen < 1:
            raise RuntimeError("construct the detector with grid_match and feed it a scan first")
        o = self._sg_out
        h = {k: getattr(o, k).cpu().numpy() for k in ("best", "score", "votes", "ok", "moved", "correction")}
        return [{"best": h["best"][b], "score": h["score"][b], "votes": int(h["votes"][b]), "ok": bool(h["ok"][b]),
                 "moved": bool(h["moved"][b]), "correction": h["correction"][b]} for b in range(self.B)], o

    def grid_refine(self):
        """-> (list with one dict per sensor of the last step's fit to the grid: correction [3] = what was added to
        (x, y, phi), score [2] = the mean interpolated grid value under the scan (before, after), obs, votes, count,
        iters_used, ok and moved;  the device-resident ``ops.GridRefine``, valid until the next call).  Needs
        ``grid_refine`` and one scan.  Synchronises."""
        if self._gr_kw is None or self._seen < 1:
            raise RuntimeError("construct the detector with grid_refine and feed it a scan first")
        o = self._gr_out
        h = {k: getattr(o, k).cpu().numpy() for k in o._fields}
        return [{"correction": h["correction"][b], "score": h["score"][b], "obs": float(h["obs"][b]),
                 "votes": int(h["votes"][b]), "count": int(h["count"][b]), "iters_used": int(h["iters_used"][b]),
                 "ok": bool(h["ok"][b]), "moved": bool(h["moved"][b])} for b in range(self.B)], o

    def grid_scroll(self):
        """-> (list with one dict per sensor of the last step's scroll: shift [2] = this step's shift in tiles of 64
        cells (x, y), scrolled, offset [2] = the shift since the reset and origin [2], the grid's lower corner now;  the
        device-resident ``ops.GridScroll``, valid until the next call).  Needs ``grid_scroll`` and one scan.
        Synchronises."""
        if self._gs_kw is None or self._seen < 1:
            raise RuntimeError("construct the detector with grid_scroll and feed it a scan first")
        o = self._gs_out
        h = {"shift": o.shift.cpu().numpy(), "scrolled": o.scrolled.cpu().numpy(),
             "offset": self._gs_state.offset.cpu().numpy(), "origin": self._gm_state.origin.cpu().numpy()}
        return [{"shift": h["shift"][b], "scrolled": bool(h["scrolled"][b]), "offset": h["offset"][b],
                 "origin": h["origin"][b]} for b in range(self.B)], o

    def grid_store(self):
        """-> (list with one dict per sensor of the last step's traffic with the tile store: restored, stored, evicted
        and dropped tiles of this step, held = the tiles in the store now, clock = the scrolls since the reset;  the
        device-resident ``ops.GridScrollStore``, valid until the next call).  Needs ``grid_store`` and one scan.
        Synchronises."""
        if self._st_kw is None or self._seen < 1:
            raise RuntimeError("construct the detector with grid_store and feed it a scan first")
        o = self._st_out
        counts, clock = o.counts.cpu().numpy(), self._st_state.clock.cpu().numpy()
        held = (self._st_state.store_stamp != 0).sum(dim=1).cpu().numpy()
        return [dict(zip(("restored", "stored", "evicted", "dropped"), (int(v) for v in counts[b])), held=int(held[b]),
                     clock=int(clock[b])) for b in range(self.B)], o

    def grid_cast(self):
        """-> the last step's ``ops.GridCast``, device-resident and valid until the next call: per beam exp_range,
        exp_far, free_range, exp_cell, exp_state and exp_steps [B,N], per point point_class [B,N] (0 none, 1 map, 2
        novel, 3 through, 4 unknown), det_novel, det_map and det_through [B,N] in the row order of ``detections()`` and
        class_count [B,5].  The grid it was cast through is the one the scans before this one left.  Needs ``grid_cast``
        and one scan.  No synchronisation: the tensors stay on the device."""
        if self._gc_kw is None or self._seen < 1:
            raise RuntimeError("construct the detector with grid_cast and feed it a scan first")
        return self._gc_out

    def novel_segments(self):
        """-> the last step's ``ops.NovelSegments``, device-resident and valid until the next call: instance_mask
        [B,N], num_det [B], det_xy [B,N,2] (sensor frame) and det_cls [B,N] in the layout of the NMS's results, det_count,
        det_first, det_last, det_width2 and det_known [B,N] per row and seg_count [B,3].  Needs ``novel_segments`` and
        one scan.  No synchronisation: the tensors stay on the device."""
        if self._ns_kw is None or self._seen < 1:
            raise RuntimeError("construct the detector with novel_segments and feed it a scan first")
        return self._ns_out

    def merged_detections(self):
        """-> the last step's ``ops.MergedDetections``, device-resident and valid until the next call: instance_mask
        [B,N], num_det [B], det_xy [B,N,2] (sensor frame) and det_cls [B,N] in the layout of the NMS's results -- the
        rows ``person_motion()``, ``tracks()`` and ``track_map()`` answer for -- det_points, det_src (1 the NMS's, 2 a
        segment) and det_row [B,N] per row, b_row, b_count and b_known [B,N] per row of ``novel_segments()`` and
        merge_count [B,4].  Needs ``merge_detections`` and one scan.  No synchronisation: the tensors stay on the
        device."""
        if self._mg_kw is None or self._seen < 1:
            raise RuntimeError("construct the detector with merge_detections and feed it a scan first")
        return self._mg_out

    def track_map(self):
        """-> (list with one list per sensor of the live tracks, in slot order as ``tracks()`` has them: dicts of id,
        cls (0 undecided, 1 free-standing, 2 unsupported, 3 background), points, free, occ (the three sums), scans,
        moved and start [2];  det_class, one array per sensor with the class of every row of ``detections()``;  the
        device-resident ``ops.TrackMapState`` and ``ops.TrackMap``, valid until the next call).  Needs ``track_map``
        and two scans of a sequence.  Reads the state back, i.e. synchronises."""
        if self._tm_kw is None or self._seen < 2:
            raise RuntimeError("construct the detector with track_map and feed it two scans of a sequence first")
        s, o = self._tm_state, self._tm_out
        h = {k: getattr(s, k).cpu().numpy() for k in s._fields}
        ids, cls = self._track_state.track_id.cpu().numpy(), o.track_class.cpu().numpy()
        det_class, counts = o.det_class.cpu().numpy(), self._person_dets()[2].cpu().numpy()
        live = [[{"id": int(ids[b, t]), "cls": int(cls[b, t]), "points": int(h["ev_points"][b, t]),
                  "free": int(h["ev_free"][b, t]), "occ": int(h["ev_occ"][b, t]), "scans": int(h["ev_scans"][b, t]),
                  "moved": bool(h["ev_moved"][b, t]), "start": h["ev_start"][b, t].copy()}
                 for t in np.flatnonzero(ids[b])] for b in range(self.B)]
        return live, [det_class[b, :m].copy() for b, m in enumerate(counts)], s, o

    def ego_motion(self):
        """-> list (one dict per sensor) of the last step's fit: motion [3] = (theta, u_x, u_y) since the previous
        scan, ok, count, rms, and pose [3], the dead-reckoned (x, y, phi) at this scan; and the device-resident
        outputs (``ops.EgoMotion``, valid until the next call).  Needs ``ego_motion`` and two scans of a sequence.
        With ``method="scan_match"`` the dicts also hold iters_used and obs, and the outputs are an ``ops.ScanMatch``.
        With ``method="keyframe"`` the motion is the one against the keyframe, the dicts also hold key_replaced,
        key_age and key_pose [3], the outputs are an ``ops.KeyframeMatch``, and one scan is enough (ok is False there).
        With ``method="keyframe_map"`` the dicts hold those and key_switched and key_slot, key_pose is the active
        slot's, and the outputs are an ``ops.KeyframeMapMatch``.
        Synchronises."""
        if self._key_kw is not None:
            if self._seen < 1:
                raise RuntimeError("feed the detector a scan first")
        elif not self._dead_reckons() or self._seen < 2:
            raise RuntimeError("construct the detector with ego_motion and feed it two scans of a sequence first")
        o = self._key_out if self._key_kw is not None else self._match_out if self._match_kw is not None \
            else self._ego_out
        row = lambda v: v
        fields = [("motion", o.motion, row), ("ok", o.ok, bool), ("count", o.count, int), ("rms", o.rms, float)]
        if self._ego_kw is None:                      # the scan matchers
            fields += [("iters_used", o.iters_used, int), ("obs", o.obs, float)]
        fields.append(("pose", self._pose_state, row))
        if self._key_kw is not None:
            s = self._key_state
            fields += [("key_replaced", o.key_replaced, bool), ("key_age", s.key_age, int), ("key_pose", s.key_pose, row)]
        if self._key_map:
            fields += [("key_switched", o.key_switched, bool), ("key_slot", o.key_slot, int)]
        host = [(k, t.cpu().numpy(), as_type) for k, t, as_type in fields]
        fits = [{k: as_type(h[b]) for k, h, as_type in host} for b in range(self.B)]
        if self._key_map:
            for fit in fits:
                fit["key_pose"] = fit["key_pose"][fit["key_slot"]]        # of the ring's poses, the active slot's
        return fits, o

    def tracks(self):
        """-> (list with one list per sensor of the live tracks, in slot order: dicts of id, xy [2], velocity [2] in
        metres per scan, cov [3] = (position variance, position/velocity covariance, velocity variance), hits,
        misses, age, confirmed and det, the row of ``person_flow()`` the track was matched with or born from in this
        step or -1;  det_track, one array per sensor with the track id of every row of ``person_flow()``;  the
        device-resident ``ops.TrackState``, valid until the next call).  Needs ``tracks`` and two scans of a sequence.
        Reads the state back, i.e. synchronises."""
        if not self._has_tracks() or self._seen < 2:
            raise RuntimeError("construct the detector with tracks and feed it two scans of a sequence first")
        s = self._track_state
        h = {k: getattr(s, k).cpu().numpy() for k in s._fields}
        counts = self._person_dets()[2].cpu().numpy()
        live = [[{"id": int(h["track_id"][b, t]), "xy": h["track_state"][b, t, :2].copy(),
                  "velocity": h["track_state"][b, t, 2:].copy(), "cov": h["track_cov"][b, t].copy(),
                  "hits": int(h["track_hits"][b, t]), "misses": int(h["track_misses"][b, t]),
                  "age": int(h["track_age"][b, t]), "confirmed": bool(h["track_confirmed"][b, t]),
                  "det": int(h["track_det"][b, t])} for t in np.flatnonzero(h["track_id"][b])] for b in range(self.B)]
        return live, [h["det_track"][b, :m].copy() for b, m in enumerate(counts)], s
