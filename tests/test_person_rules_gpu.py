"""The scenes of tests/test_person_rules.py on the GPU: pof_person_motion with its rules, ties and gates taken by rows of
the later register slots, across the 63 | 64 and 511 | 512 ownership boundaries and in the last slot of either kernel
form; pof_track_update with ties between the slots of one lane, the gate at equality and at 0, max_misses = 0, a slot
that looks again three times, and candidates behind the first staged chunk; the base weights of pof_ego_motion at
equality.  The referees are the float64 restatements the older tests use -- person_motion_oracle, track_step,
base_weights -- through the comparison helpers of those tests: every person-motion field bit for bit (a NaN equals any
NaN), the tracker's integers equal and its float state within that file's 1e-12 (the helper prints whether the bits
agree), the ego-motion fit within the tolerance tests/test_ego_motion.py derives, its count and weights exactly."""
import numpy as np
import pytest
import torch

import test_person_motion_gpu as PM
import test_person_rules as S
import test_tracks_gpu as TR
from test_ego_motion import assert_matches, base_weights, tolerance
from test_person_motion import DEFAULTS, STATE_FIELDS, axis_table, motion_state, person_motion_oracle, rule_scans, same_bits, tie_scans

pytestmark = pytest.mark.gpu

FIELDS = PM.FIELDS + STATE_FIELDS


@pytest.fixture(scope="module")
def ops():
    from planar_optical_flow_amd import ops as _ops
    return _ops


def on_device(ops, scans, what, **kw):
    """One placed sequence (AxisScans) through the device and the restatement, every field the same bits.
    -> the device's outputs per scan, of the one sensor."""
    got = PM.check_sequences(ops, [[s.inputs() for s in scans]], axis_table(scans[0].N), what, **kw)
    return [{k: v[0] for k, v in g.items()} for g in got]


shifted = lambda want, at: [j + at if j >= 0 else -1 for j in want]


# ------------------------------------------------------------------ 1. person motion beyond a thread's first slot
@pytest.mark.parametrize("N,at", S.PLACEMENTS2)
def test_two_point_rule_and_tie_scenes_at_later_rows(ops, N, at):
    what = "N=%d at=%d " % (N, at)
    got = on_device(ops, S.embed(rule_scans(), at, N), what + "rules", **S.KW2)
    assert list(got[1]["det_prev"][at:at + 8]) == shifted(S.RULE_PREV[0], at) == shifted([-1, 0, -1, -1, -1, 4, -1, 5], at)
    assert list(got[2]["det_prev"][at:at + 3]) == shifted(S.RULE_PREV[1], at)
    assert np.array_equal(got[1]["det_prev"][:at], np.arange(at)) and np.array_equal(got[2]["det_prev"][:at], np.arange(at))
    got = on_device(ops, S.embed(rule_scans(), at, N), what + "rules, far", **dict(S.KW2, reach=0.75))
    assert list(got[1]["det_prev"][at:at + 8]) == shifted(S.RULE_PREV_FAR, at) and np.array_equal(got[1]["det_flow"][at], [0.75, 0.0])
    got = on_device(ops, S.embed(rule_scans(), at, N), what + "rules, loose", **dict(S.KW2, min_points=1, cls_thresh=0.1))
    assert list(got[1]["det_prev"][at:at + 8]) == shifted(S.RULE_PREV_LOOSE[0], at)
    assert list(got[2]["det_prev"][at:at + 3]) == shifted(S.RULE_PREV_LOOSE[1], at)
    got = on_device(ops, S.embed(tie_scans()["previous rows"], at, N), what + "tie/previous rows", **S.KW2)
    assert got[1]["det_prev"][at] == at + 1 and np.array_equal(got[1]["det_flow"][at], [-0.25, 0.0])
    got = on_device(ops, S.embed(tie_scans()["current rows"], at, N), what + "tie/current rows", **S.KW2)
    assert list(got[1]["det_prev"][at:at + 3]) == [-1, at, -1] and np.array_equal(got[1]["det_flow"][at + 1], [0.0, 0.25])


@pytest.mark.parametrize("N,at", S.PLACEMENTS1)
def test_single_point_scene_at_later_rows_and_in_the_last_slot(ops, N, at):
    what = "N=%d at=%d " % (N, at)
    got = on_device(ops, S.embed(S.point_scans(), at, N, 1), what + "points", **S.KW1)
    assert list(got[1]["det_prev"][at:at + 10]) == shifted(S.POINT_PREV[0], at) == shifted([-1, 0, -1, -1, -1, 3, 4, -1, 5, 6], at)
    assert list(got[2]["det_prev"][at:at + 2]) == shifted(S.POINT_PREV[1], at)
    assert np.array_equal(got[1]["det_prev"][:at], np.arange(at))
    for k, f in S.POINT_FLOW.items():
        assert np.array_equal(got[1]["det_flow"][at + k], f), k
    got = on_device(ops, S.embed(S.point_scans(), at, N, 1), what + "points, far", **dict(S.KW1, reach=0.75))
    assert list(got[1]["det_prev"][at:at + 10]) == shifted(S.POINT_PREV_FAR, at) and np.array_equal(got[1]["det_flow"][at], [0.75, 0.0])


@pytest.mark.parametrize("N,at", S.GATE_PLACEMENTS)
def test_score_threshold_and_max_range_at_equality(ops, N, at):
    got = on_device(ops, S.embed(S.gate_scans(), at, N, 1), "N=%d at=%d gates" % (N, at), **S.KW1)
    assert list(got[1]["det_prev"][at:at + 4]) == shifted(S.GATE_PREV[0], at) == [at, -1, at + 2, -1]
    assert list(got[2]["det_prev"][at:at + 2]) == shifted(S.GATE_PREV[1], at) == [-1, at + 1]
    assert list(got[0]["det_valid"][at:at + 4]) == [1, 0, 1, 1] and list(got[1]["det_valid"][at:at + 4]) == [1, 1, 1, 0]
    assert list(got[1]["det_count"][at:at + 4]) == [1, 1, 1, 1]
    assert np.array_equal(got[1]["det_centre"][at + 2], [S.MAX_RANGE - 0.0625, 0.0])


@pytest.mark.parametrize("N,lo,hi", S.BOUNDARY_TIES)
def test_ties_across_an_ownership_boundary(ops, N, lo, hi):
    seqs = [[s.inputs() for s in S.boundary_tie(kind, N, lo, hi)] for kind in ("previous", "current")]
    got = PM.check_sequences(ops, seqs, axis_table(N), "N=%d ties at rows %d | %d" % (N, lo, hi), **S.KW2)[1]
    want = np.arange(hi + 1)
    want[hi] = -1
    for b, flow in ((0, [-0.25, 0.0]), (1, [0.0, 0.25])):
        assert np.array_equal(got["det_prev"][b][:hi + 1], want), b
        assert np.array_equal(got["det_flow"][b][lo], flow) and np.isnan(got["det_flow"][b][hi]).all()


@pytest.mark.parametrize("N,j,k_lo,k_hi", S.MUTUALS)
def test_mutual_rule_between_slots(ops, N, j, k_lo, k_hi):
    got = on_device(ops, S.mutual_scene(N, j, k_lo, k_hi), "N=%d mutual %d <- %d, %d" % (N, j, k_lo, k_hi), **S.KW2)[1]
    assert got["det_prev"][k_hi] == j and got["det_prev"][k_lo] == -1 and np.array_equal(got["det_flow"][k_hi], [0.125, 0.0])


@pytest.mark.parametrize("N,big,small", S.SLOT_COUNTS)
def test_scans_of_different_slot_counts(ops, N, big, small):
    got = on_device(ops, S.slot_count_scans(N, big, small), "N=%d rows %d, %d, %d" % (N, big, small, big), **S.KW2)
    assert [int(g["prev_num"]) for g in got] == [big, small, big]
    assert np.array_equal(got[1]["det_prev"][:small], big - 1 - np.arange(small))         # partners beyond num_det
    assert np.array_equal(got[2]["det_prev"][:big], np.where(np.arange(big) >= big - small, big - 1 - np.arange(big), -1))


def _dense(N):
    return PM.crowd_seq(N, 2, N, seed=N, min_points=1)


@pytest.mark.parametrize("N", [128, 1024])
def test_a_state_and_a_count_from_a_longer_scan_are_clamped(ops, N):
    """tests/test_person_motion.test_clamped_counts_and_a_state_from_a_longer_scan on the device, with every row of the
    previous scan a detection: prev_num = N + 1000 reads as N, num_det = N + 7 as N."""
    tab, seq = _dense(N)
    kw = dict(DEFAULTS, min_points=1, reach=1.0)
    state, out, ref = ops.person_motion_state(1, N), ops.person_motion_buffers(1, N), motion_state(N)
    want = None
    for t, s in enumerate(seq):
        s = dict(s, num_det=np.int32(N + 7 * t))
        ops.person_motion(*PM._inputs([s], tab), state, out=out, **kw)
        want = person_motion_oracle(s["ranges"], tab, s["inst"], s["num_det"], s["det_xy"], s["det_cls"], s["rot"], s["trans"],
                                    ref, **kw)
        if t == 0:
            state.prev_num.fill_(N + 1000)
            ref["prev_num"][...] = N + 1000
    got = PM._host(out, state)
    want.update(ref)
    for k in FIELDS:
        assert same_bits(got[k][0], np.asarray(want[k], got[k].dtype)), k
    T = S.threads_of(N)
    assert int(got["prev_num"][0]) == N and (got["det_prev"][0][T:] >= 0).any() and (got["det_prev"][0] >= T).any()


@pytest.mark.parametrize("N", [128, 512, 513, 4096])
def test_every_beam_its_own_detection(ops, N):
    """num_det = N, single-point rows, permuted between the scans: every register slot of either form is full.
    Measured on an MI355X host: 0.2 s for N = 4096, nearly all of it the restatement, so both scans stay."""
    tab, seq = _dense(N)
    got = PM.check_sequences(ops, [seq], tab, "N=%d, %d detections" % (N, N), min_points=1, reach=1.0)[-1]
    T, prev = S.threads_of(N), got["det_prev"][0]
    last = (N - 1) // T * T                                    # the first row of the last slot in use
    assert got["prev_num"][0] == N and ((prev[last:] >= 0).any() or (prev >= last).any()) and (prev[:T] >= T).any()
    if N - last >= 64:                                         # N = 513 has one row in its last slot
        assert (prev[last:] >= 0).any() and (prev >= last).any()
    assert (prev < 0).sum() >= N // 20 and (got["det_count"][0] == 0).any() and (got["det_valid"][0] == 0).any()


# ------------------------------------------------------------------ 2. tracker
@pytest.mark.parametrize("name", sorted(S.track_scenes()))
def test_tracker_scenes(ops, name):
    M, N, seq, kw, expect = S.track_scenes()[name]
    got = TR.check_sequences(ops, [seq], M, N, name, **kw)
    sensor = [{k: v[0] for k, v in g.items()} for g in got]
    S.check_expectations(sensor[-1], expect, name, steps=sensor)
    if name == "max_misses 0":
        assert [int(g["track_id"][0, 0]) for g in got] == [1, 2] and [int(g["dropped"][0]) for g in got] == [0, 0]
    if name == "same lane/128":
        assert list(got[-1]["track_det"][0, [1, 65]]) == [0, -1] and list(got[-1]["track_misses"][0, [1, 65]]) == [0, 1]


# ------------------------------------------------------------------ 3. ego-motion base weights at equality
@pytest.mark.parametrize("N", [8, 513])
def test_ego_motion_base_weights_at_equality(ops, N):
    c = S.ego_equality_case(N)
    w0 = base_weights(c["xy"], c["flow"], weight=c["weight"], ranges=c["ranges"], inst=c["inst"], num=c["num"],
                      det_cls=c["det_cls"])
    tol, want = tolerance([((c["xy"], c["flow"], w0, -1, 0), {})])
    cuda = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt)[None])).cuda()
    out = ops.ego_motion(cuda(c["ranges"], np.float32), None, cuda(c["flow"], np.float64), xy=cuda(c["xy"], np.float64),
                         canonical=False, weight=cuda(c["weight"], np.float32), instance_mask=cuda(c["inst"], np.int32),
                         num_det=cuda(c["num"], np.int32), det_cls=cuda(c["det_cls"], np.float64), cls_thresh=0.5,
                         max_range=20.0, iters=0)
    got = {k: getattr(out, k)[0].cpu().numpy() for k in out._fields}
    assert_matches(got, want[0], tol, N)
    assert int(got["count"]) == int((w0 > 0).sum()) == N - 4 and int(got["ok"]) == 1
    assert np.array_equal(got["weight"] == 0, w0 == 0) and np.array_equal(got["weight"], w0.astype(np.float32))
    for name, i in c["at"].items():
        assert (got["weight"][i] > 0) == c["counted"][name], name
    assert got["weight"][c["at"]["tiny weight"]] == np.float32(2.0 ** -149)


# ------------------------------------------------------------------ 4. the same bits anywhere, again and in a graph
def test_person_motion_scene_at_five_batch_positions_twice_and_replayed(ops):
    N, kw = 1024, S.KW1
    tab = axis_table(N)
    seq = lambda scans: [s.inputs() for s in scans]
    a = seq(S.embed(S.point_scans(), 505, N, 1))
    others = [seq(S.embed(S.point_scans(), 300, N, 1)), seq(S.embed(S.gate_scans(), 510, N, 1)), seq(S.embed(S.point_scans(), 0, N, 1))]
    seqs = [a, others[0], a, others[1], a, others[2], a, a]
    first, again, alone = (PM.dev_steps(ops, s, tab, **kw) for s in (seqs, seqs, [a]))
    for t in range(3):
        for k in FIELDS:
            assert same_bits(first[t][k], again[t][k]), k
            for b in (0, 2, 4, 6, 7):
                assert same_bits(first[t][k][b], alone[t][k][0]), (k, b)
    assert list(alone[1]["det_prev"][0][505:515]) == shifted(S.POINT_PREV[0], 505)
    assert not np.array_equal(first[1]["det_prev"][0], first[1]["det_prev"][1])
    bufs = [torch.zeros_like(t) for t in PM._inputs([s[0] for s in seqs], tab)]
    state, out = ops.person_motion_state(8, N), ops.person_motion_buffers(8, N)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.person_motion(*bufs, ops.person_motion_state(8, N), **kw)          # warm-up on a state of its own
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.person_motion(*bufs, state, out=out, **kw)
    ops.person_motion_reset(state)
    for t in range(3):
        for dst, src in zip(bufs, PM._inputs([s[t] for s in seqs], tab)):
            dst.copy_(src)
        graph.replay()
        got = PM._host(out, state)
        for k in FIELDS:
            assert same_bits(got[k], first[t][k]), (t, k)


def test_tracker_chain_at_five_batch_positions_twice_and_replayed(ops):
    scenes = S.track_scenes()
    M, N, a, kw, expect = scenes["chain 4/2049"]
    others = [scenes["chain 3/2049"][2], [a[0], S.second_scan(N, {}, rows=N)], scenes["chain 3/2049"][2][::-1]]
    seqs = [a, others[0], a, others[1], a, others[2], a, a]
    first, again, alone = (TR.dev_steps(ops, s, M, N, **kw) for s in (seqs, seqs, [a]))
    for t in range(2):
        TR._same_bits(first[t], again[t])
        for k in TR.FIELDS:
            for b in (0, 2, 4, 6, 7):
                assert np.array_equal(first[t][k][b], alone[t][k][0]), (k, b)
    S.check_expectations({k: v[0] for k, v in alone[-1].items()}, expect, "chain, alone")
    assert not np.array_equal(first[-1]["track_det"][0], first[-1]["track_det"][1])
    bufs = [torch.zeros_like(t) for t in TR._inputs([s[0] for s in seqs])]
    captured = ops.track_buffers(8, M, N)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.track_update(*bufs, ops.track_buffers(8, M, N), **kw)              # warm-up on a state of its own
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.track_update(*bufs, captured, **kw)
    ops.track_reset(captured)
    for t in range(2):
        for dst, src in zip(bufs, TR._inputs([s[t] for s in seqs])):
            dst.copy_(src)
        graph.replay()
        TR._same_bits(TR._host(captured), first[t])
