"""The Python layer of the per-scan stages N5-N12 without a GPU and without the library: every record of tensors
``ops`` declares, and every setting and default ``ops`` and ``StreamingDetector`` expose, against literal tables.

The tables were written down from the code before the records had one declaration form and the settings one source
(each ``*_buffers`` / ``*_state`` function run on the CPU at the sizes below, each wrapper's ``inspect.signature``), so
they hold the declarations to what the C entry points have always been handed: the namedtuples are unpacked
positionally into the call, and a field out of order, of another dtype or with a transposed shape would be a wrong
pointer, not an error."""
import pytest
import torch

from planar_optical_flow_amd import ops, streaming

B, N, K, M, H, W = 2, 5, 3, 4, 64, 128          # pairwise distinct: a transposed shape cannot pass
f32, f64, i32, i16, u8 = torch.float32, torch.float64, torch.int32, torch.int16, torch.uint8
_FIT = (("motion", f64, (2, 3)), ("count", i32, (2,)), ("rms", f64, (2,)), ("ok", u8, (2,)))
_ICP = _FIT + (("iters_used", i32, (2,)), ("obs", f64, (2,)))
_POINTS = (("corr", i32, (2, 5)), ("flow_residual", f64, (2, 5, 2)))
# function: (its arguments, the record's class name, (field, dtype, shape) in order)
RECORDS = {
    "person_flow_buffers": ((B, N), "PersonFlow", (
        ("flow_global", f32, (2, 5, 2)), ("flow_world", f64, (2, 5, 2)), ("rgb", f64, (2, 5, 3)),
        ("det_xy_world", f64, (2, 5, 2)), ("det_flow", f64, (2, 5, 2)), ("det_rgb", f64, (2, 5, 3)),
        ("det_count", i32, (2, 5)), ("det_valid", u8, (2, 5)))),
    "ego_motion_buffers": ((B, N), "EgoMotion", _FIT + (("flow_residual", f64, (2, 5, 2)), ("weight", f32, (2, 5)))),
    "scan_match_buffers": ((B, N), "ScanMatch", _ICP + _POINTS),
    "keyframe_buffers": ((B, N), "KeyframeState", (
        ("key_ranges", f32, (2, 5)), ("key_pose", f64, (2, 3)), ("key_rel", f64, (2, 3)), ("key_valid", u8, (2,)),
        ("key_age", i32, (2,)), ("key_misses", i32, (2,)), ("pose", f64, (2, 3)))),
    "keyframe_match_buffers": ((B, N), "KeyframeMatch", _ICP + (("key_replaced", u8, (2,)),) + _POINTS),
    "keyframe_map_buffers": ((B, N, K), "KeyframeMapState", (
        ("key_ranges", f32, (2, 3, 5)), ("key_pose", f64, (2, 3, 3)), ("key_valid", u8, (2, 3)),
        ("key_stamp", i32, (2, 3)), ("key_active", i32, (2,)), ("key_rel", f64, (2, 3)), ("key_age", i32, (2,)),
        ("key_misses", i32, (2,)), ("step", i32, (2,)), ("pose", f64, (2, 3)))),
    "keyframe_map_match_buffers": ((B, N), "KeyframeMapMatch", _ICP + (
        ("key_replaced", u8, (2,)), ("key_switched", u8, (2,)), ("key_slot", i32, (2,))) + _POINTS),
    "track_buffers": ((B, M, N), "TrackState", (
        ("track_id", i32, (2, 4)), ("track_state", f64, (2, 4, 4)), ("track_cov", f64, (2, 4, 3)),
        ("track_hits", i32, (2, 4)), ("track_misses", i32, (2, 4)), ("track_age", i32, (2, 4)), ("next_id", i32, (2,)),
        ("track_det", i32, (2, 4)), ("track_confirmed", u8, (2, 4)), ("det_track", i32, (2, 5)),
        ("point_track", i32, (2, 5)), ("dropped", i32, (2,)))),
    "person_motion_buffers": ((B, N), "PersonMotion", (
        ("det_xy_world", f64, (2, 5, 2)), ("det_flow", f64, (2, 5, 2)), ("det_centre", f64, (2, 5, 2)),
        ("det_count", i32, (2, 5)), ("det_valid", u8, (2, 5)), ("det_prev", i32, (2, 5)))),
    "person_motion_state": ((B, N), "PersonMotionState", (
        ("prev_centre", f64, (2, 5, 2)), ("prev_cand", u8, (2, 5)), ("prev_num", i32, (2,)))),
    "grid_map_buffers": ((B, N), "GridMapOut", (
        ("point_cell", i32, (2, 5)), ("point_mark", u8, (2, 5)), ("point_prior", i16, (2, 5)),
        ("det_points", i32, (2, 5)), ("det_free", i32, (2, 5)))),
    "grid_map_state": ((B, H, W), "GridMapState", (("grid", i16, (2, 64, 128)), ("origin", f64, (2, 2)))),
}

_SCAN_MATCH = dict(cls_thresh=0.5, max_range=20.0, window=16, gate=0.5, max_gap=0.3, huber_delta=0.05, iters=16,
                   eps_theta=1e-7, eps_u=1e-7, min_pivot=1e-6)
_KEYFRAME = dict(_SCAN_MATCH, key_dist=0.3, key_rot=0.3, min_share=0.5, max_misses=2)
SETTINGS = {
    "ego_motion": dict(canonical=True, sign=-1, model="rigid", cls_thresh=0.5, max_range=20.0, huber_delta=0.0,
                       iters=0),
    "scan_match": _SCAN_MATCH,
    "keyframe_match": _KEYFRAME,
    "keyframe_map_match": dict(_KEYFRAME, revisit=0.5),
    "track_update": dict(gate=0.5, q=1e-4, r_pos=2.5e-3, r_vel=2.5e-3, v0_var=0.25, max_misses=3, min_hits=3),
    "person_motion": dict(cls_thresh=0.5, max_range=20.0, reach=0.5, min_points=3),
    "grid_map_update": dict(cls_thresh=0.5, max_range=20.0, tol=None, hit=17, miss=8, lo=-40, hi=70, free_thresh=16,
                            res=ops.REQUIRED),
}
# what a StreamingDetector with cls_thresh = 0.7 accepts per constructor argument (and ego_motion method)
_TRACKS = dict(SETTINGS["track_update"], max_tracks=64)
_GRID = dict(max_range=20.0, tol=None, hit=17, miss=8, lo=-40, hi=70, free_thresh=16, res=0.1, size=512)
DETECTOR = {
    ("ego_motion", "flow"): dict(huber_delta=0.02, iters=4, max_range=20.0, cls_thresh=0.7),
    ("ego_motion", "scan_match"): dict(_SCAN_MATCH, cls_thresh=0.7),
    ("ego_motion", "keyframe"): dict(_KEYFRAME, cls_thresh=0.7),
    ("ego_motion", "keyframe_map"): dict(_KEYFRAME, cls_thresh=0.7, keys=16, revisit=0.5),
    ("tracks", "flow"): _TRACKS,
    ("person_motion", "flow"): dict(max_range=20.0, reach=0.5, min_points=3),
    ("grid_map", "flow"): _GRID,
}


def test_records_are_what_the_entry_points_take():
    for fn, (args, cls, fields) in RECORDS.items():
        rec = getattr(ops, fn)(*args, device="cpu")
        assert type(rec) is getattr(ops, cls) and type(rec).__name__ == cls, fn
        assert rec._fields == tuple(f for f, _, _ in fields), fn
        for (f, dtype, shape), t in zip(fields, rec):
            assert (t.dtype, tuple(t.shape), t.device.type) == (dtype, shape, "cpu"), (fn, f)
            if (fn, f) != ("track_buffers", "next_id"):
                assert not t.any(), (fn, f)
    tracks = ops.track_buffers(B, M, N, device="cpu")
    assert tracks.next_id.tolist() == [1, 1]
    assert ops.TrackState.persistent == ("track_id", "track_state", "track_cov", "track_hits", "track_misses",
                                         "track_age", "next_id")


def test_settings_and_defaults_have_one_source():
    for name, want in SETTINGS.items():
        got = ops.stage_settings(getattr(ops, name))
        assert got == want and {k: type(v) for k, v in got.items()} == {k: type(v) for k, v in want.items()}, name
    for (arg, method), want in DETECTOR.items():
        assert streaming.stage_defaults(arg, 0.7, method) == want, (arg, method)
        assert streaming.stage_settings(arg, {}, 0.7, method) == want, (arg, method)
        given = {next(iter(want)): 3}
        assert streaming.stage_settings(arg, given, 0.7, method) == dict(want, **given), (arg, method)
        unknown = "cls_thresh" if arg in ("person_motion", "grid_map") else "no_such_setting"
        with pytest.raises(ValueError, match="unknown %s settings" % arg):
            streaming.stage_settings(arg, {unknown: 0.5}, 0.7, method)


def test_grid_shape_is_the_rule_of_the_four_launchers():
    """``ops.grid_shape`` (what the detector and ``OccupancyGrid`` check a ``size`` with) and the launchers' shape rule
    (csrc/pof_grid.h) accept the same sides.  B = 0: a launcher returns in front of any launch, so no pointer is
    followed and no GPU is needed; every other argument is legal, so POF_E_SHAPE can only come from H and W."""
    import ctypes
    import os
    from planar_optical_flow_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH) and not os.path.exists(build.HIPCC):
        pytest.skip("the library is not built and there is no hipcc to build it")
    build.build(verbose=False)
    lib = _lib.load()
    buf = (ctypes.c_char * 32)()
    word = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)     # non-null and 16-byte aligned

    def w(n):
        return [word] * n

    launchers = {
        "pof_grid_map_update": lambda H, W: lib.pof_grid_map_update(*w(7), 0.1, 0.1, 20.0, 0.5, 17, 8, -40, 70, 16, 0, 8,
                                                                    H, W, *w(7), None),
        "pof_grid_match": lambda H, W: lib.pof_grid_match(*w(5), 0.5, 20.0, word, word, 0.1, word, 4, 9, 50, 20, 8, 0, 8,
                                                          H, W, *w(10), None),
        "pof_grid_scroll": lambda H, W: lib.pof_grid_scroll(word, 0.1, 0, 0, H, W, *w(7), None),
        "pof_grid_cast": lambda H, W: lib.pof_grid_cast(*w(9), 0.1, 20.0, 0.1, 17, 16, 0, 8, H, W, *w(11), None),
    }
    seen = set()
    for side in (-64, 0, 32, 63, 64, 96, 128, 2048, 2112, 4096):
        for H, W in ((side, 64), (64, side)):
            try:
                assert ops.grid_shape((H, W)) == (H, W)
                want = _lib.POF_OK
            except ValueError:
                want = _lib.POF_E_SHAPE
            seen.add(want)
            for name, call in launchers.items():
                assert call(H, W) == want, (name, H, W)
        # one number is the square of it
        if want == _lib.POF_OK:
            assert ops.grid_shape(side) == (side, side)
        else:
            with pytest.raises(ValueError):
                ops.grid_shape(side)
    assert seen == {_lib.POF_OK, _lib.POF_E_SHAPE}
