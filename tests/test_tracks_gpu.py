"""Person tracks (pof_track_update, N7) on the GPU: against the NumPy restatement of tests/test_tracks.py on its
scenarios -- integers and flags equal at every step, the float state within 1e-12 m (the fixed operation order is
expected to give the same bits; the tests print whether it does) -- at the sizes where the launch changes form, at
the limits, in a captured graph and as the tail of the streaming detector."""
import os
import sys

import numpy as np
import pytest
import torch

from test_tracks import (FLOAT_FIELDS, INT_FIELDS, OUTPUTS, PERSISTENT, SETTINGS, crowd_sequence, excluded_rows_sequence,
                         ids_of, lifecycle_sequence, run_steps, scan_of, tie_sequences, walkers)

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "planar_optical_flow_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

FIELDS = PERSISTENT + OUTPUTS
STATE_TOL = 1e-12


@pytest.fixture(scope="module")
def ops():
    from planar_optical_flow_amd import ops as _ops
    return _ops


def _inputs(scans):
    """One step's inputs of B sensors (dicts of tests/test_tracks.scan_of) as device tensors."""
    stack = lambda k, dt: torch.from_numpy(np.ascontiguousarray(np.stack([s[k] for s in scans]), dtype=dt)).cuda()
    return (stack("xy", np.float64), stack("flow", np.float64), stack("valid", np.uint8), stack("num_det", np.int32),
            stack("inst", np.int32))


def _host(state):
    return {k: getattr(state, k).cpu().numpy() for k in FIELDS}


def dev_steps(ops, seqs, M, N, **kw):
    """The device's states after every step; seqs: one sequence per sensor, all of one length."""
    state = ops.track_buffers(len(seqs), M, N)
    out = []
    for scans in zip(*seqs):
        ops.track_update(*_inputs(scans), state, **kw)
        out.append(_host(state))
    return out


def assert_equals_restatement(got, want, b, what):
    """-> whether the float state has the same bits, too."""
    for k in INT_FIELDS:
        assert np.array_equal(got[k][b], want[k]), (what, k)
    for k in FLOAT_FIELDS:
        assert np.isfinite(got[k][b]).all(), (what, k)
        assert np.abs(got[k][b] - want[k]).max(initial=0.0) <= STATE_TOL, (what, k)
    return all(np.array_equal(got[k][b], want[k]) for k in FLOAT_FIELDS)


def check_sequences(ops, seqs, M, N, what, **kw):
    got = dev_steps(ops, seqs, M, N, **kw)
    same = True
    for b, seq in enumerate(seqs):
        for t, want in enumerate(run_steps(seq, M, N, **kw)):
            same &= assert_equals_restatement(got[t], want, b, (what, b, t))
    print("%s: float state %s the restatement's bits" % (what, "has" if same else "is within 1e-12 of, but has not,"))
    return got


def _same_bits(a, b):
    for k in FIELDS:
        assert np.array_equal(a[k], b[k]), k


# ------------------------------------------------------------------ 1. the crossing scenario
def test_crossing_scenario_three_sensors_against_the_restatement(ops):
    seqs, rows = [], []
    for b in range(3):
        seq, r, _ = walkers(100 + b, N=16, variant=b)
        seqs.append(seq)
        rows.append(r)
    got = check_sequences(ops, seqs, 64, 16, "crossing", **SETTINGS)
    for b in range(3):                                         # and the scenario's truth, on the device's own output
        ids = ids_of([{"det_track": g["det_track"][b]} for g in got], rows[b])
        assert all(len(set(col[col > 0])) == 1 for col in ids.T)
    assert not np.array_equal(got[-1]["track_state"][0], got[-1]["track_state"][1])


# ------------------------------------------------------------------ 2. launch forms and limits
def _crowd(n_valid, N, seed, steps=3):
    """n_valid people among N rows (the others are not valid) who drift; in the later steps every seventh is missed
    and the rows are permuted."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(max(n_valid, 1))))
    home = np.stack([(np.arange(n_valid) % side) * 1.5, (np.arange(n_valid) // side) * 1.5], axis=1)
    vel = rng.uniform(-0.1, 0.1, (n_valid, 2))
    seq = []
    for t in range(steps):
        seen = np.flatnonzero((np.arange(n_valid) % 7 != 3) | (t == 0))
        order = rng.permutation(N)[:len(seen)] if t else np.arange(len(seen))
        s = scan_of(np.zeros((N, 2)), N=N, valid=np.zeros(N, np.uint8), inst=rng.integers(0, N + 2, N))
        s["xy"][:] = rng.uniform(-50, 50, (N, 2))              # rows that are not valid hold something
        s["xy"][order] = home[seen] + vel[seen] * t + rng.normal(0, 0.02, (len(seen), 2))
        s["flow"][order] = vel[seen] + rng.normal(0, 0.03, (len(seen), 2))
        s["valid"][order] = 1
        seq.append(s)
    return seq


@pytest.mark.parametrize("M", [1, 63, 64, 65, 256])
def test_slot_counts_and_candidate_counts(ops, M):
    for n_valid in (0, 1, 64, 65):
        got = check_sequences(ops, [_crowd(n_valid, 80, seed=M + n_valid)], M, 80, "M=%d, %d valid rows" % (M, n_valid),
                              **SETTINGS)
        assert got[0]["dropped"][0] == max(0, n_valid - M) and got[0]["next_id"][0] == 1 + min(M, n_valid)


def test_all_450_rows_valid(ops):
    got = check_sequences(ops, [_crowd(450, 450, seed=3), _crowd(450, 450, seed=4)], 256, 450, "450 valid rows", **SETTINGS)
    assert (got[0]["dropped"] == 450 - 256).all() and (got[-1]["track_id"] > 0).all()


def _largest():
    """N = 4096 with every row a candidate: a 64 x 64 grid of people 1 m apart.  In the second scan everyone has
    moved 0.4375 m along x and every fourth of the first 256 is missed, so with a gate of 0.625 m the track of a missed
    person first looks at its left neighbour's detection (0.5625 m away), loses it to that neighbour and looks again:
    the second look of a scan with more than one staged chunk."""
    grid = np.stack([np.arange(4096) % 64, np.arange(4096) // 64], axis=1).astype(np.float64)
    first = scan_of(grid, N=4096, inst=np.arange(4096) % 4099)
    valid = np.ones(4096, np.uint8)
    valid[np.arange(5, 256, 4)] = 0
    second = scan_of(grid + [0.4375, 0.0], N=4096, valid=valid, inst=(np.arange(4096) * 7) % 4099)
    return [first, second]


def test_largest_scan_every_row_a_candidate(ops):
    kw = dict(SETTINGS, gate=0.625)
    got = check_sequences(ops, [_largest()], 256, 4096, "N=4096, 4096 candidates", **kw)
    assert got[0]["dropped"][0] == 4096 - 256 and got[1]["dropped"][0] == 4096 - 256      # nobody left, so no slot
    assert (got[1]["track_misses"][0][np.arange(5, 256, 4)] == 1).all() and got[1]["track_misses"][0].sum() == 63


def test_one_past_each_limit_is_refused_and_nothing_is_touched(ops):
    from planar_optical_flow_amd._lib import POF_E_SHAPE, PofError
    for M, N in ((257, 64), (64, 4097)):
        seq = _crowd(40, N, seed=9, steps=1)
        state = ops.track_buffers(1, M, N)
        for t in state:                                        # a state and outputs that are not zeros
            t.copy_(torch.from_numpy(np.random.default_rng(1).integers(1, 100, tuple(t.shape))).to(t.dtype))
        before = _host(state)
        with pytest.raises(PofError) as e:
            ops.track_update(*_inputs(seq[:1]), state, **SETTINGS)
        assert e.value.code == POF_E_SHAPE
        _same_bits(_host(state), before)
    with pytest.raises(ValueError):
        ops.track_update(*_inputs(_crowd(4, 8, seed=1, steps=1)), ops.track_buffers(1, 4, 9), **SETTINGS)
    with pytest.raises(AssertionError):
        ops.track_update(*_inputs(_crowd(4, 8, seed=1, steps=1)), ops.track_buffers(1, 4, 8), **dict(SETTINGS, r_pos=0.0))
    empty = ops.track_buffers(0, 4, 8)
    assert ops.track_update(*(t[:0] for t in _inputs(_crowd(4, 8, seed=1, steps=1))), empty).track_id.shape == (0, 4)


# ------------------------------------------------------------------ 3. ties, excluded rows, lifecycle
def test_ties_on_the_device(ops):
    kw = dict(SETTINGS, gate=2.5)
    for name, (M, N, seq) in tie_sequences().items():
        got = check_sequences(ops, [seq], M, N, "tie/" + name, **kw)[-1]
        if name == "rows":
            assert got["track_det"][0, 0] == 1
        elif name == "slots":
            assert list(got["track_det"][0, :2]) == [0, -1]
        else:
            assert [got["track_det"][0, t] for t in (1, 2, 63, 64, 65)] == [1, -1, 0, 2, -1]


def test_excluded_rows_nan_flow_and_lifecycle_on_the_device(ops):
    got = check_sequences(ops, [excluded_rows_sequence()], 4, 6, "excluded rows", **SETTINGS)
    assert list(got[1]["det_track"][0]) == [0, 0, 0, 0, 1, 0]
    assert list(got[2]["track_cov"][0, 1]) == [SETTINGS["r_pos"], 0.0, SETTINGS["v0_var"]]
    got = check_sequences(ops, [lifecycle_sequence()], 1, 4, "lifecycle", **SETTINGS)
    assert [int(g["track_id"][0, 0]) for g in got] == [1, 1, 1, 1, 2, 2]
    got = check_sequences(ops, [crowd_sequence()], 5, 8, "crowd", **SETTINGS)
    assert all(g["dropped"][0] == 2 for g in got) and list(got[-1]["track_confirmed"][0]) == [1] * 5
    # reset: everything free again, ids from 1
    state = ops.track_buffers(1, 5, 8)
    ops.track_update(*_inputs(crowd_sequence()[:1]), state, **SETTINGS)
    assert ops.track_reset(state) is not None and int(state.next_id[0]) == 1 and not state.track_id.any()
    ops.track_update(*_inputs(crowd_sequence()[:1]), state, **SETTINGS)
    assert list(state.track_id[0].cpu().numpy()) == [1, 2, 3, 4, 5]


# ------------------------------------------------------------------ 4. determinism
@pytest.mark.parametrize("M", [64, 256])
def test_a_sensor_gives_the_same_bits_at_every_batch_position_and_in_every_run(ops, M):
    seqs = [walkers(200 + b, N=16, variant=b % 5)[0][:8] for b in range(69)]
    seqs.append(seqs[0])
    batch, again, alone = (dev_steps(ops, s, M, 16, **SETTINGS) for s in (seqs, seqs, seqs[:1]))
    for t in range(8):
        _same_bits(batch[t], again[t])
        for k in FIELDS:
            assert np.array_equal(batch[t][k][0], batch[t][k][69]) and np.array_equal(batch[t][k][0], alone[t][k][0]), k
    assert not np.array_equal(batch[-1]["track_state"][0], batch[-1]["track_state"][1])


# ------------------------------------------------------------------ 5. graph
def test_captured_update_replays_bit_identically(ops):
    B, M, N = 2, 64, 16
    seqs = [walkers(300 + b, N=N, variant=b)[0] for b in range(B)]
    bufs = [torch.zeros_like(t) for t in _inputs([s[0] for s in seqs])]
    captured, eager = ops.track_buffers(B, M, N), ops.track_buffers(B, M, N)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.track_update(*bufs, ops.track_buffers(B, M, N), **SETTINGS)       # warm-up on a state of its own
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.track_update(*bufs, captured, **SETTINGS)
    ops.track_reset(captured)                                  # the capture itself runs nothing; start from scratch
    for t in range(5):
        for dst, src in zip(bufs, _inputs([s[t] for s in seqs])):
            dst.copy_(src)
        graph.replay()
        ops.track_update(*bufs, eager, **SETTINGS)
        _same_bits(_host(captured), _host(eager))
    assert (captured.track_age.max(dim=1).values == 4).all() and (captured.next_id >= 7).all()


# ------------------------------------------------------------------ 6. the reference-shaped wrapper
def test_person_tracker_wrapper(ops):
    import src.utils.utils as u
    seq, rows, _ = walkers(100, N=16)
    want = run_steps(seq, 32, 16, **SETTINGS)
    tracker = u.PersonTracker(max_tracks=32, **SETTINGS)
    for t, s in enumerate(seq[:6]):
        m = int(s["num_det"])
        ids, tracks = tracker.update({"dets_xy_world": s["xy"][:m], "person_flow": s["flow"][:m],
                                      "valid": s["valid"][:m].astype(bool), "instance_mask": s["inst"]})
        live = np.flatnonzero(want[t]["track_id"])
        assert np.array_equal(ids, want[t]["det_track"][:m]) and np.array_equal(tracks["id"], want[t]["track_id"][live])
        assert np.array_equal(tracks["point_track"], want[t]["point_track"])
        assert np.abs(tracks["velocity"] - want[t]["track_state"][live, 2:]).max() <= STATE_TOL
        assert np.array_equal(tracks["det"], want[t]["track_det"][live])
    ids, tracks = tracker.update({"dets_xy_world": np.zeros((0, 2)), "person_flow": np.zeros((0, 2)), "valid": np.zeros(0, bool)})
    assert len(ids) == 0 and (tracks["misses"] == 1).all() and "point_track" not in tracks
    tracker.reset()
    ids, _ = tracker.update({"dets_xy_world": np.ones((1, 2)), "person_flow": np.zeros((1, 2)), "valid": np.ones(1, bool)})
    assert list(ids) == [1]
    with pytest.raises(ValueError):
        u.PersonTracker(gates=1.0)


# ------------------------------------------------------------------ 7. streaming detector
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
    from planar_optical_flow_amd import synth
    scans = torch.from_numpy(synth.make_batch(seed=seed, B=B, T=T).scans).cuda()
    flows = torch.from_numpy(np.random.default_rng(seed).normal(0, 0.03, (T, B, 450, 2)).astype(np.float32)).cuda()
    return scans, flows


def _tracks_equal(a, b):
    (la, da, sa), (lb, db, sb) = a, b
    assert len(la) == len(lb)
    for ta, tb in zip(la, lb):
        assert len(ta) == len(tb)
        for x, y in zip(ta, tb):
            assert x.keys() == y.keys()
            for k in x:
                assert np.array_equal(x[k], y[k]), k
    assert all(np.array_equal(x, y) for x, y in zip(da, db))
    _same_bits(_host(sa), _host(sb))


@pytest.mark.parametrize("ego", [False, True])
@pytest.mark.parametrize("B", [1, 2])
def test_streaming_detector_graph_and_eager_keep_the_same_tracks(B, ego):
    from planar_optical_flow_amd.streaming import StreamingDetector
    T = 6
    model, stub = _stream_model(13), _BufferFlow(B, 450).cuda()
    scans, flows = _sequence(B, T, seed=61 + B)
    kw = dict(batch=B, nms_min_dist=0.5, flow_model=stub, cls_thresh=0.0,        # every detection is a candidate
              tracks=dict(max_tracks=64, gate=1.0, min_hits=2, max_misses=10))
    if ego:
        kw["ego_motion"] = dict(cls_thresh=2.0)
    eager, graphed = StreamingDetector(model, graph=False, **kw), StreamingDetector(model, graph=True, **kw)

    def run():
        for t in range(T):
            stub.flow.copy_(flows[t])
            eager(scans[:, t]), graphed(scans[:, t])
            if t == 0:
                for det in (eager, graphed):
                    with pytest.raises(RuntimeError):
                        det.tracks()
                continue
            te, tg = eager.tracks(), graphed.tracks()
            _tracks_equal(te, tg)
            live, det_track, state = tg
            counts = graphed._dets[2].cpu().numpy()
            for b in range(B):
                assert len(det_track[b]) == counts[b]
                assert max(tr["age"] for tr in live[b]) == t - 1           # the warm-up did not advance the state
                assert sorted(tr["id"] for tr in live[b] if tr["det"] >= 0) == sorted(det_track[b][det_track[b] > 0])
        return tg

    live, _, state = run()
    assert graphed._graph is not None and eager._graph is None
    assert all(len(l) > 0 for l in live) and int(state.next_id.min()) > 1
    assert any(tr["confirmed"] for l in live for tr in l)
    first_ids = [sorted(tr["id"] for tr in l) for l in live]
    eager.reset(), graphed.reset()
    assert int(graphed._track_state.next_id.max()) == 1 and not graphed._track_state.track_id.any()
    with pytest.raises(RuntimeError):
        graphed.tracks()
    live, _, _ = run()                                         # the same sequence again: ids restart at 1
    assert [sorted(tr["id"] for tr in l) for l in live] == first_ids and min(min(i) for i in first_ids) >= 1


def test_streaming_detector_without_tracks_is_the_parent_step():
    from planar_optical_flow_amd.streaming import StreamingDetector
    B, T = 2, 3
    model, stub = _stream_model(13), _BufferFlow(B, 450).cuda()
    scans, flows = _sequence(B, T, seed=67)
    kw = dict(batch=B, nms_min_dist=0.5, flow_model=stub)
    plain, none, tracked = (StreamingDetector(model, **kw), StreamingDetector(model, tracks=None, **kw),
                            StreamingDetector(model, tracks=dict(), **kw))
    for det in (plain, none):
        assert not any("track" in name and not callable(getattr(det, name)) for name in dir(det))
        with pytest.raises(RuntimeError):
            det.tracks()
    assert tracked._track_state.track_id.shape == (B, 64)
    for t in range(T):
        stub.flow.copy_(flows[t])
        outs = [tuple(o.clone() for o in det(scans[:, t])) for det in (plain, none, tracked)]
        for other in outs[1:]:
            assert all(torch.equal(x, y) for x, y in zip(outs[0], other))
        if t:
            flows_ = [det.person_flow()[1] for det in (plain, none, tracked)]
            for other in flows_[1:]:
                for k in other._fields:
                    assert np.array_equal(getattr(flows_[0], k).cpu().numpy(), getattr(other, k).cpu().numpy(), equal_nan=True), k
    with pytest.raises(ValueError):
        StreamingDetector(model, batch=B, nms_min_dist=0.5, tracks=dict())                    # needs flow_model
    with pytest.raises(ValueError):
        StreamingDetector(model, tracks=dict(gates=1.0), **kw)
