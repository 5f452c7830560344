"""The tile store behind the scrolling grid (pof_grid_scroll_store, N20) on the GPU: the device against the NumPy
restatement of tests/test_grid_store.py, BIT FOR BIT in every state field (grid, origin, offset, store, store_key,
store_stamp, clock) and every output (shift, scrolled, counts) behind every call -- integers and bitwise copies behind
N14's one float64 expression per axis: no tolerance and no excluded case -- on the rule scenes, at five batch positions
and in two runs, with 1024 tiles leaving for 1024 and 1023 slots, in a captured launch, in a chain with the grid update
out and back, on refused calls, through ``utils.OccupancyGrid`` and as a stage of the streaming detector."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from test_grid_map import DEFAULTS as MAP_DEFAULTS, OUT_FIELDS as MAP_FIELDS, ambiguous_cells, grid_map_oracle
from test_grid_scroll import grid_scroll_oracle, rule_scenes as scroll_scenes, run_scene as run_scroll_scene
from test_grid_store import (EXPECTED, RES, WINDOW, WINDOW_MARGIN, WINDOW_RANGE, CHAIN_SLOTS, chain, copy_store,
                             device_scenes, empty_store, grid_scroll_store_oracle, rule_scenes, run_scene)
from test_scan_match import angle_table, make_room, ray_cast

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "planar_optical_flow_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

STATE = ("grid", "origin", "offset", "tiles", "key", "stamp", "clock")
FIELDS = STATE + ("shift", "scrolled", "counts")


@pytest.fixture(scope="module")
def ops():
    from planar_optical_flow_amd import ops as _ops
    return _ops


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _setup(ops, scene, sensors):
    """The device state of a batch of sensors as the scene gives it; the workspaces and the outputs hold sentinels: what
    a workspace holds means nothing, and the outputs are always written."""
    B, H, W, S = len(sensors), scene["H"], scene["W"], scene["S"]
    state, scroll = ops.grid_map_state(B, H, W), ops.grid_scroll_state(B, H, W)
    store, out = ops.grid_store_state(B, H, W, S), ops.grid_scroll_store_buffers(B)
    stores = [s["store"] if "store" in s else empty_store(S) for s in sensors]
    state.grid.copy_(_dev(np.stack([s["grid"] for s in sensors]), np.int16))
    state.origin.copy_(_dev(np.stack([s["origin"] for s in sensors]), np.float64))
    scroll.base.copy_(_dev(np.stack([s["base"] for s in sensors]), np.float64))
    scroll.offset.copy_(_dev(np.stack([s["offset"] for s in sensors]), np.int32))
    store.store.copy_(_dev(np.stack([st["tiles"] for st in stores]), np.int16))
    store.store_key.copy_(_dev(np.stack([st["key"] for st in stores]), np.int32))
    store.store_stamp.copy_(_dev(np.stack([st["stamp"] for st in stores]), np.int32))
    store.clock.copy_(_dev(np.concatenate([st["clock"] for st in stores]), np.int32))
    scroll.scratch.fill_(12345)
    store.plan_in.fill_(-7)
    store.plan_out.fill_(1 << 20)
    for t in out:
        t.fill_(99)
    return state, scroll, store, out


def _host(state, scroll, store, out):
    return {"grid": state.grid.cpu().numpy(), "origin": state.origin.cpu().numpy(), "offset": scroll.offset.cpu().numpy(),
            "base": scroll.base.cpu().numpy(), "tiles": store.store.cpu().numpy(), "key": store.store_key.cpu().numpy(),
            "stamp": store.store_stamp.cpu().numpy(), "clock": store.clock.cpu().numpy()[:, None],
            "shift": out.shift.cpu().numpy(), "scrolled": out.scrolled.cpu().numpy(), "counts": out.counts.cpu().numpy()}


def dev_steps(ops, scene, want, sensors=None):
    """The device's state and outputs behind every call, the sensors in one batch; the positions are the ones the
    restatement was given (``want``: its per-sensor lists of calls)."""
    sensors = scene["sensors"] if sensors is None else sensors
    state, scroll, store, out = _setup(ops, scene, sensors)
    res = []
    for k in range(len(want[0])):
        trans = _dev(np.stack([w[k]["trans"] for w in want]), np.float64)
        got = ops.grid_scroll_store(trans, state, scroll, store, res=scene["res"], margin=scene["margin"], out=out)
        assert got is out
        res.append(_host(state, scroll, store, out))
    return res


def same_bits(g, w, b, what):
    """Sensor b of a device step against a call of the restatement, every state field and every output."""
    for f in FIELDS:
        assert g[f][b].dtype == np.asarray(w[f]).dtype, (what, f)
        assert np.array_equal(g[f][b], w[f]), (what, f)
    assert g["origin"][b].tobytes() == w["origin"].tobytes(), what


def check_scene(ops, scene, what):
    want = run_scene(scene)
    got = dev_steps(ops, scene, want)
    for b, (s, calls) in enumerate(zip(scene["sensors"], want)):
        for k, w in enumerate(calls):
            same_bits(got[k], w, b, (what, b, k))
            assert got[k]["base"][b].tobytes() == s["base"].tobytes()          # read only
    return got


# ------------------------------------------------------------------ 1. the device against the restatement
@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_rule_scenes(ops, name):
    scene = rule_scenes()[name]
    got = check_scene(ops, scene, name)
    answers = [[(tuple(int(v) for v in g["shift"][b]), tuple(int(v) for v in g["counts"][b])) for g in got]
               for b in range(len(scene["sensors"]))]
    assert answers == [list(e) for e in EXPECTED[name]]        # the literal table, on the device


@pytest.mark.parametrize("name", sorted(device_scenes()))
def test_all_tiles_of_the_largest_grid_leave(ops, name):
    scene = device_scenes()[name]
    got = check_scene(ops, scene, name)[-1]
    S = scene["S"]
    assert got["counts"][0, 1] == S and got["counts"][0, 3] == 1024 - S and not got["grid"].any()


def test_n14s_scenes_give_n14s_bits(ops):
    """Everything N14 writes is N14's: its own rule scenes through the storing entry point -- the grid too until a
    tile returns (in "256 cap" and "256 away and back" a column does)."""
    returned = set()
    for name, scene in scroll_scenes().items():
        want = run_scroll_scene(scene)
        got = dev_steps(ops, dict(scene, S=3), want)
        for b, calls in enumerate(want):
            restored = 0
            for k, w in enumerate(calls):
                restored += int(got[k]["counts"][b, 0])
                for f in ("offset", "shift", "scrolled") + (("grid",) if not restored else ()):
                    assert np.array_equal(got[k][f][b], w[f]), (name, b, k, f)
                assert got[k]["origin"][b].tobytes() == w["origin"].tobytes(), (name, b, k)
            if restored:
                returned.add(name)
    assert returned == {"256 cap", "256 away and back"}


# ------------------------------------------------------------------ 2. determinism
@pytest.mark.parametrize("embedded", ["128 released and reused", "128 eviction, two leave"])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_same_bits_at_every_batch_position_and_in_two_runs(ops, B, embedded):
    """One scene as one sensor among copies of the other: a restore with an eviction in the same call among calls that
    only store, and the other way round."""
    scenes = rule_scenes()
    scene = scenes["128 released and reused"]
    me, other = scene["sensors"][0], dict(scenes["128 eviction, two leave"]["sensors"][0])
    other["store"] = {k: v[:3] if k != "clock" else v for k, v in other["store"].items()}      # three slots, as ``me``
    if embedded != "128 released and reused":
        me, other = other, me
    want_me = run_scene(dict(scene, sensors=[me]))[0]
    want_other = run_scene(dict(scene, sensors=[other]))[0]
    runs = {}
    for pos in [p for p in (0, 1, 2, 3, 4) if p < B] + [B // 2]:
        sensors, want = [other] * B, [want_other] * B
        sensors[pos], want[pos] = me, want_me
        got = dev_steps(ops, scene, want, sensors)
        for k in range(len(want_me)):
            for b in range(B):
                same_bits(got[k], want[b][k], b, (B, pos, b, k))
        runs.setdefault(pos, []).append(got)
    first, second = runs[B // 2]                               # the two runs at one position: every sensor's bits
    for f in FIELDS:
        assert all(np.array_equal(a[f], b[f]) for a, b in zip(first, second)), f


def test_a_captured_launch_replayed_out_and_back(ops):
    scene = rule_scenes()["192x256 y only"]
    s = scene["sensors"][0]
    # six positions as cells of the grid as it stands: up, up, stay, back, back, stay
    steps = [(130, 128), (130, 128), (130, 100), (130, 63), (130, 63), (130, 100)]
    want = run_scene(dict(scene, sensors=[dict(s, steps=steps)]))
    assert [tuple(c["shift"]) for c in want[0]] == [(0, 1), (0, 1), (0, 0), (0, -1), (0, -1), (0, 0)]
    assert [int(c["counts"][0]) for c in want[0]] == [0, 0, 0, 4, 4, 0]
    state, scroll, store, out = _setup(ops, scene, [s])
    trans = torch.zeros((1, 2), dtype=torch.float64, device="cuda")
    kw = dict(res=scene["res"], margin=scene["margin"], out=out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                              # a launch in front of the capture: nothing lazy is left
        ops.grid_scroll_store(trans + 1e9, state, scroll, store, **kw)      # |c| >= 2^30: no shift
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.grid_scroll_store(trans, state, scroll, store, **kw)
    # the capture ran nothing; put the scene's state in place and replay
    fresh = _setup(ops, scene, [s])
    for mine, new in zip(tuple(state) + tuple(scroll) + tuple(store), tuple(fresh[0]) + tuple(fresh[1]) + tuple(fresh[2])):
        mine.copy_(new)
    for k, w in enumerate(want[0]):
        trans.copy_(_dev(w["trans"][None], np.float64))
        graph.replay()
        same_bits(_host(state, scroll, store, out), w, 0, ("replay", k))
    assert _host(state, scroll, store, out)["grid"][0].tobytes() == s["grid"].tobytes()        # out and back: every bit


# ------------------------------------------------------------------ 3. a chain with the grid update
def test_out_and_back_with_the_grid_update_equals_the_restatement(ops):
    tab, scans, poses, base, steps = chain()
    state, scroll = ops.grid_map_state(1, WINDOW, WINDOW), ops.grid_scroll_state(1, WINDOW, WINDOW)
    store, out = ops.grid_store_state(1, WINDOW, WINDOW, CHAIN_SLOTS), ops.grid_scroll_store_buffers(1)
    ops.grid_scroll_reset(scroll, ops.grid_map_reset(state, base))
    tab_d = _dev(tab, np.float64)
    kw = {k: v for k, v in dict(MAP_DEFAULTS, max_range=WINDOW_RANGE).items()}
    restored = 0
    for t, w in enumerate(steps):
        rot, trans = _dev(w["rot"].reshape(1, 2, 2), np.float32), _dev(w["trans"][None], np.float64)
        ops.grid_scroll_store(trans, state, scroll, store, res=RES, margin=WINDOW_MARGIN, out=out)
        g = _host(state, scroll, store, out)
        for f in ("origin", "offset", "shift", "scrolled", "counts", "clock", "key", "stamp"):
            assert np.array_equal(g[f][0], w[f]), (t, f)
        assert ambiguous_cells(tab, w["rot"], w["trans"], g["origin"][0], RES, WINDOW, WINDOW, WINDOW_RANGE) == 0
        m = ops.grid_map_update(_dev(scans[t][None], np.float32), tab_d, rot, trans, state, res=RES, **kw)
        for k in MAP_FIELDS:
            assert np.array_equal(getattr(m, k)[0].cpu().numpy(), w["map"][k]), (t, k)
        assert np.array_equal(state.grid[0].cpu().numpy(), w["grid"]), t
        assert np.array_equal(store.store[0].cpu().numpy(), w["tiles"]), t
        restored += int(g["counts"][0, 0])
    assert restored >= 2


# ------------------------------------------------------------------ 4. refused calls
def _raw(ops, trans, state, scroll, store, out, slots, res=0.1, margin=0, null=None, store_shift=0):
    """The entry point itself, past the wrapper's checks -> its return code."""
    from planar_optical_flow_amd import _lib
    from planar_optical_flow_amd.ops import _ptr, _stream
    B, H, W = state.grid.shape
    ptrs = [_ptr(t) for t in tuple(state) + tuple(scroll) + tuple(store) + tuple(out)]
    if store_shift:
        ptrs[5] = ctypes.c_void_p(store.store.data_ptr() + store_shift)
    if null is not None:
        ptrs[null] = None
    return getattr(_lib.load(), "pof_grid_scroll_store")(_ptr(trans), float(res), int(margin), int(slots), B, H, W, *ptrs,
                                                         _stream())


def test_refused_calls_leave_state_and_outputs_untouched(ops):
    from planar_optical_flow_amd._lib import POF_E_BADARG, POF_E_SHAPE, PofError
    rng = np.random.default_rng(1)
    H = W = 256
    state, scroll = ops.grid_map_state(1, H, W), ops.grid_scroll_state(1, H, W)
    store, out = ops.grid_store_state(1, H, W, 4), ops.grid_scroll_store_buffers(1)
    tensors = tuple(state) + tuple(scroll) + tuple(store) + tuple(out)
    for t in tensors:                                          # sentinels
        t.copy_(torch.from_numpy(rng.integers(1, 100, tuple(t.shape))).to(t.dtype))
    before = [t.cpu().numpy() for t in tensors]
    trans = _dev([[1000.0, -1000.0]], np.float64)              # far outside: a call that went through would scroll
    raw = [(dict(slots=0), POF_E_BADARG), (dict(slots=1025), POF_E_BADARG), (dict(slots=-1), POF_E_BADARG),
           (dict(slots=4, store_shift=8), POF_E_SHAPE), (dict(slots=4, store_shift=2), POF_E_SHAPE),
           (dict(slots=4, margin=65), POF_E_BADARG), (dict(slots=4, res=0.0), POF_E_BADARG)]
    raw += [(dict(slots=4, null=k), POF_E_BADARG) for k in range(5, 14)]       # the store's pointers and the outputs
    for kw, code in raw:
        assert _raw(ops, trans, state, scroll, store, out, **kw) == code, kw
    for kw, error in ((dict(margin=65), AssertionError), (dict(margin=-1), AssertionError),
                      (dict(res=0.0), AssertionError), (dict(res=float("nan")), AssertionError)):
        with pytest.raises(error):                             # N14's own, through the wrapper
            ops.grid_scroll_store(trans, state, scroll, store, out=out, **dict(dict(res=0.1, margin=0), **kw))
    small = ops.grid_map_state(1, 64, 96)
    with pytest.raises(PofError) as e:
        ops.grid_scroll_store(trans, small, ops.grid_scroll_state(1, 64, 96), ops.grid_store_state(1, 64, 128, 4)[:4] +
                              (torch.zeros((1, 1), dtype=torch.int32, device="cuda"),) * 2, res=0.1, margin=0)
    assert e.value.code == POF_E_SHAPE
    torch.cuda.synchronize()
    after = [t.cpu().numpy() for t in tensors]
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    # the wrapper's own refusals
    ok_state, ok_scroll, ok_store = ops.grid_map_state(1, H, W), ops.grid_scroll_state(1, H, W), ops.grid_store_state(1, H, W, 4)
    zero = _dev([[0.0, 0.0]], np.float64)
    with pytest.raises(ValueError):
        ops.grid_scroll_store(zero, ok_state, ok_scroll, ops.grid_store_state(2, H, W, 4), res=0.1)        # another batch
    with pytest.raises(ValueError):
        ops.grid_scroll_store(zero, ok_state, ok_scroll, ops.grid_store_state(1, H, 128, 4), res=0.1)      # another grid
    with pytest.raises(ValueError):
        ops.grid_scroll_store(zero, ok_state, ok_scroll, ok_store, res=0.1, out=ops.grid_scroll_store_buffers(2))
    with pytest.raises(TypeError):
        ops.grid_scroll_store(zero.float(), ok_state, ok_scroll, ok_store, res=0.1)
    empty = ops.grid_scroll_store(zero[:0], ops.grid_map_state(0, 64, 64), ops.grid_scroll_state(0, 64, 64),
                                  ops.grid_store_state(0, 64, 64, 4), res=0.1)
    assert empty.counts.shape == (0, 4)
    # the next good call works on the very tensors the refused ones were given, sentinels and all: the window is
    # emptied, 16 tiles leave for 4 slots, and the stamps decide which slot takes which
    h = _host(state, scroll, store, out)
    grid, origin, offset = h["grid"][0].copy(), h["origin"][0].copy(), h["offset"][0].copy()
    st = dict(tiles=h["tiles"][0].copy(), key=h["key"][0].copy(), stamp=h["stamp"][0].copy(), clock=h["clock"][0].copy())
    want = grid_scroll_store_oracle(trans.cpu().numpy()[0], grid, origin, h["base"][0], offset, st, 0.1, 0)
    assert want["counts"].tolist() == [0, 4, 4, 12]
    ops.grid_scroll_store(trans, state, scroll, store, res=0.1, margin=0, out=out)
    same_bits(_host(state, scroll, store, out), dict(want, grid=grid, origin=origin, offset=offset, **st), 0, "after the refusals")
    # grid_store_reset empties the store with tensor ops
    for t in store:
        t.fill_(3)
    ops.grid_store_reset(store)
    assert not store.store_stamp.any() and not store.clock.any()


# ------------------------------------------------------------------ 5. the reference-shaped wrapper
def test_occupancy_grid_wrapper_equals_the_direct_calls(ops):
    import src.utils.utils as u
    tab_np, scans, poses, base, steps = chain()
    N = len(scans[0])
    phi = tab_np[:N]
    og = u.OccupancyGrid(phi, res=RES, size=WINDOW, max_range=WINDOW_RANGE, scroll=dict(margin=WINDOW_MARGIN), store=dict(slots=8))
    plain = u.OccupancyGrid(phi, res=RES, size=WINDOW, max_range=WINDOW_RANGE, scroll=dict(margin=WINDOW_MARGIN))
    assert plain._store is None and plain.store_tiles == 0 and og._store.store.shape == (1, 8, 64, 64)
    with pytest.raises(ValueError, match="give both"):
        u.OccupancyGrid(phi, store=dict(slots=8))
    tab = u._table_for(phi)
    first = poses[0][:2] - 0.5 * RES * np.array([WINDOW, WINDOW], np.float64)  # the first pose in the middle
    state = ops.grid_map_state(1, WINDOW, WINDOW)
    scroll = ops.grid_scroll_reset(ops.grid_scroll_state(1, WINDOW, WINDOW), ops.grid_map_reset(state, first))
    store = ops.grid_store_state(1, WINDOW, WINDOW, 8)
    restored = 0
    for t, scan in enumerate(scans):
        got, still = og.update(scan, poses[t]), plain.update(scan, poses[t])
        rot, trans, _ = u._pose_terms(poses[t][None])
        rot, trans = torch.from_numpy(rot).cuda(), torch.from_numpy(trans).cuda()
        s = ops.grid_scroll_store(trans, state, scroll, store, res=RES, margin=WINDOW_MARGIN)
        o = ops.grid_map_update(torch.from_numpy(scan).cuda().reshape(1, N), tab, rot, trans, state, res=RES,
                                max_range=WINDOW_RANGE)
        assert np.array_equal(got["shift"], s.shift[0].cpu().numpy()) and np.array_equal(still["shift"], got["shift"])
        assert np.array_equal(got["store_counts"], s.counts[0].cpu().numpy()) and "store_counts" not in still
        for k in ("point_cell", "point_prior"):
            assert np.array_equal(got[k], getattr(o, k)[0].cpu().numpy()), (t, k)
        assert np.array_equal(og.logodds, state.grid[0].cpu().numpy()) and np.array_equal(og.offset, scroll.offset[0].cpu().numpy())
        assert og.store_tiles == int((store.store_stamp != 0).sum())
        restored += int(got["store_counts"][0])
    assert restored >= 2 and not np.array_equal(og.logodds, plain.logodds)
    og.reset()
    assert og.store_tiles == 0 and not og._store.clock.any() and not og.logodds.any()


# ------------------------------------------------------------------ 6. streaming detector
def _stream_model(seed):
    from planar_optical_flow_amd.src.depracted.model.dr_spaam import SpatialDROW
    torch.manual_seed(seed)
    return SpatialDROW(num_scans=5, num_pts=56, alpha=0.5, window_size=11, pedestrian_only=True).cuda().eval()


STREAM_OUT, STREAM_PAST, STREAM_SIZE, STREAM_RES, STREAM_RANGE, STREAM_SLOTS = 12, 4, 256, 0.02, 6.0, 16
STREAM_BEGIN = (0.213, -0.127)


def two_drives_out_and_back(seed=81, N=450):
    """Two sensors, each in a room of its own, driven straight from STREAM_BEGIN, back over the same poses and four
    steps past the start (a dead-reckoned pose may lag the true one): sensor 0 along +x at 0.25 m per scan, sensor 1
    along -y at 0.27 m per scan, turning by 0.01 rad per scan, 12 scans out and 16 back.  A 256 x 256 grid of 0.02 m cells with margin 64 scrolls 64 cells = 1.28 m from its middle: sensor 0 goes up a
    tile twice and comes back two tiles at once some 1.5 m into the way back, sensor 1 goes down two tiles at once and
    comes back one some 1.7 m into the way back; either return restores what was stored.  -> (scans float32 [T,2,N], poses [T,2,3])."""
    rng = np.random.default_rng(seed)
    phi = angle_table(N)[:N]
    T = 2 * STREAM_OUT + STREAM_PAST
    scans, poses = np.zeros((T, 2, N), np.float32), np.zeros((T, 2, 3))
    for b, (course, step, heading) in enumerate(((0.0, 0.25, 0.3), (-0.5 * np.pi, 0.27, -1.2))):
        segs = make_room(rng)
        for t in range(T):
            k = t if t < STREAM_OUT else 2 * STREAM_OUT - 1 - t
            poses[t, b] = (STREAM_BEGIN[0] + np.cos(course) * step * k, STREAM_BEGIN[1] + np.sin(course) * step * k,
                           heading + 0.01 * k)
            scans[t, b] = (ray_cast(segs, poses[t, b], phi) + rng.normal(0.0, 1.0, N) * 0.01).astype(np.float32)
    return scans, poses


def _snapshot(det, store):
    """Everything the scroll and the grid stage read and leave behind, on the host."""
    _, conf, num, inst = det._dets
    state, out = det.grid_map()
    snap = {"pred_cls": det.pred_cls, "det_cls": conf, "num_det": num, "inst": inst, "rot": det._pose_rot,
            "trans": det._pose_trans, "grid": state.grid, "origin": state.origin, "shift": det._gs_out.shift,
            "scrolled": det._gs_out.scrolled, "offset": det._gs_state.offset}
    snap.update({k: getattr(out, k) for k in MAP_FIELDS})
    if store:
        st = det._st_state
        snap.update(counts=det._st_out.counts, tiles=st.store, key=st.store_key, stamp=st.store_stamp, clock=st.clock)
    return {k: v.detach().cpu().numpy().copy() for k, v in snap.items()}


@pytest.mark.parametrize("ego", ["keyframe", "scan_match"])
def test_streaming_detector_eager_graph_and_restatement(ego):
    from planar_optical_flow_amd.streaming import StreamingDetector
    B, size, res = 2, STREAM_SIZE, STREAM_RES
    scans, poses = two_drives_out_and_back()
    T = len(scans)
    model = _stream_model(13)
    kw = dict(batch=B, nms_min_dist=0.5, cls_thresh=0.5, ego_motion=dict(method=ego),
              grid_map=dict(size=size, res=res, max_range=STREAM_RANGE), grid_scroll=dict())
    eager = StreamingDetector(model, graph=False, grid_store=dict(slots=STREAM_SLOTS), **kw)
    graphed = StreamingDetector(model, graph=True, grid_store=dict(slots=STREAM_SLOTS), **kw)
    parent = StreamingDetector(model, graph=True, **kw)          # what the detector was without the store
    assert parent._st_kw is None and not hasattr(parent, "_st_state") and not hasattr(parent, "_st_out")
    assert len(eager._stages) == len(parent._stages)             # the same table: the scroll's entry stores
    names = [getattr(s.launch, "__name__", "") for s in graphed._stages]
    assert names == [getattr(s.launch, "__name__", "") for s in parent._stages] and names.count("_grid_scroll_stage") == 1
    at = names.index("_grid_scroll_stage")                       # the store's four persistent fields join its snapshot
    assert len(graphed._stages[at].state) == len(parent._stages[at].state) + 4
    with pytest.raises(ValueError, match="give both"):
        StreamingDetector(model, grid_map=dict(size=size), grid_store=dict(slots=4))
    with pytest.raises(ValueError):
        StreamingDetector(model, grid_map=dict(size=size), grid_scroll=dict(), grid_store=dict(slots=0))
    tab = graphed.tab.cpu().numpy()
    settings = dict(MAP_DEFAULTS, max_range=STREAM_RANGE)
    half = 0.5 * res * size
    start = poses[0][:, :2]

    def run(fresh):
        grids = [np.zeros((size, size), np.int16) for _ in range(B)]
        plains = [np.zeros((size, size), np.int16) for _ in range(B)]
        origins, offsets = [start[b] - half for b in range(B)], [np.zeros(2, np.int32) for _ in range(B)]
        p_origins, p_offsets = [o.copy() for o in origins], [o.copy() for o in offsets]
        stores, totals = [empty_store(STREAM_SLOTS) for _ in range(B)], np.zeros((B, 4), np.int64)
        for det in (eager, graphed, parent):
            det.reset(pose=poses[0])
            if det is not parent:
                assert not det._st_state.store_stamp.any() and not det._st_state.clock.any()
                with pytest.raises(RuntimeError):
                    det.grid_store()
        for t in range(T):
            for det in (eager, graphed, parent):
                det(torch.from_numpy(scans[t]).cuda())
            e, g, p = _snapshot(eager, True), _snapshot(graphed, True), _snapshot(parent, False)
            for k in e:
                assert np.array_equal(e[k], g[k]), (t, k)      # eager and replayed: identical bits, store included
            for b in range(B):
                want = grid_scroll_store_oracle(g["trans"][b], grids[b], origins[b], start[b] - half, offsets[b], stores[b], res)
                for f in ("shift", "scrolled", "counts"):
                    assert np.array_equal(g[f][b], want[f]), (t, b, f)
                assert np.array_equal(g["offset"][b], offsets[b]) and g["origin"][b].tobytes() == origins[b].tobytes(), (t, b)
                # behind a reset() the free slots hold what they held: cells and keys mean nothing without a stamp
                held = slice(None) if fresh else stores[b]["stamp"] != 0
                for f in ("tiles", "key"):
                    assert np.array_equal(g[f][b][held], stores[b][f][held]), (t, b, f)
                assert np.array_equal(g["stamp"][b], stores[b]["stamp"]) and g["clock"][b] == stores[b]["clock"][0], (t, b)
                totals[b] += want["counts"]
                assert ambiguous_cells(tab, g["rot"][b], g["trans"][b], g["origin"][b], res, size, size, STREAM_RANGE) == 0
                m = grid_map_oracle(scans[t, b], tab, g["rot"][b], g["trans"][b], grids[b], origins[b], res, g["inst"][b],
                                    g["num_det"][b], g["det_cls"][b], **settings)
                for k in MAP_FIELDS:
                    assert np.array_equal(g[k][b], m[k]), (t, b, k)
                assert np.array_equal(g["grid"][b], grids[b]), (t, b)
            # a detector without the store has the parent's bits: N14 and the grid update on its own pose terms
            for b in range(B):
                grid_scroll_oracle(p["trans"][b], plains[b], p_origins[b], start[b] - half, p_offsets[b], res)
                assert ambiguous_cells(tab, p["rot"][b], p["trans"][b], p["origin"][b], res, size, size, STREAM_RANGE) == 0
                grid_map_oracle(scans[t, b], tab, p["rot"][b], p["trans"][b], plains[b], p_origins[b], res, p["inst"][b],
                                p["num_det"][b], p["det_cls"][b], **settings)
                assert np.array_equal(p["grid"][b], plains[b]) and np.array_equal(p["offset"][b], p_offsets[b]), (t, b)
            if not totals[:, 0].any():                         # up to the first restore: the parent's outputs
                for k in p:
                    assert np.array_equal(p[k], g[k]), (t, k)
        dicts, rec = graphed.grid_store()
        assert rec is graphed._st_out and len(dicts) == B
        for b, d in enumerate(dicts):
            assert [d[k] for k in ("restored", "stored", "evicted", "dropped")] == g["counts"][b].tolist()
            assert d["held"] == int((stores[b]["stamp"] != 0).sum()) and d["clock"] == int(stores[b]["clock"][0])
        shifts, rec = graphed.grid_scroll()
        assert rec is graphed._gs_out and type(rec) is type(parent.grid_scroll()[1])
        assert all(np.array_equal(shifts[b]["shift"], g["shift"][b]) for b in range(B))
        return totals, [gr.copy() for gr in grids], [copy_store(s) for s in stores]

    totals, grids, stores = run(True)
    lag = np.hypot(*(graphed._pose_trans.cpu().numpy() - poses[-1][:, :2]).T)
    print("ego=%s: tiles restored, stored, evicted, dropped per sensor %s; offsets %s; the last pose is %s m from the true one"
          % (ego, totals.tolist(), graphed._gs_state.offset.cpu().numpy().tolist(), np.round(lag, 3).tolist()))
    assert (totals[:, 0] >= 1).all() and (totals[:, 1] >= 2).all()   # each sensor stores and gets tiles back
    assert graphed._graph is not None and eager._graph is None
    again = run(False)                                         # the same sequence again behind a reset
    assert np.array_equal(again[0], totals) and all(np.array_equal(a, b) for a, b in zip(again[1], grids))
    for a, b in zip(again[2], stores):
        assert all(np.array_equal(a[f], b[f]) for f in ("tiles", "key", "stamp", "clock"))      # the restatement's own
