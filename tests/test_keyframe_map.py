"""The keyframe map (pof_keyframe_map_match, N10) without a GPU: ``keyframe_map_oracle`` is the float64 NumPy restatement
of the N10 comment in include/pof_abi.h for one sensor and one step on explicit state.  The matcher is the one of
tests/test_scan_match.py (``_iterate``) around the window centres of tests/test_keyframe.py; only the ring of keyframes
and its policy are new.  It is run here against ``keyframe_oracle`` with one slot (bit for bit), on every branch of the
policy with the state asserted field by field, on paths that return to where they began, and under N8's
summation-order / decision-margin rule.  tests/test_keyframe_map_gpu.py imports the helpers below.

Drift on a return (``test_a_return_drops_the_drift_of_the_way_round``): six committed seeds per path; the figures the
restatement gives on them are printed by the test and quoted in DESIGN 8, N10."""
import inspect
import math

import numpy as np
import pytest

from oracle import ref_numpy as R
from test_ego_motion import seq_sum
from test_keyframe import (SETTINGS, SEEDS, _centres, compose, keyframe_oracle, new_state, scenario, sequence)
from test_scan_match import (MARGIN_MIN, _Margins, _iterate, add_people, angle_table, corridor, make_room, person_points,
                             ray_cast)

MAP = dict(SETTINGS, revisit=0.5)
TAB = angle_table(450)


# ---------------------------------------------------------------- the restatement: one sensor, one step
def new_map_state(N, keys, pose=(0.0, 0.0, 0.0)):
    """The state of a sensor without a keyframe, as ops.keyframe_map_buffers / keyframe_map_reset leave it."""
    return dict(key_ranges=np.zeros((keys, N), np.float32), key_pose=np.zeros((keys, 3)), key_valid=np.zeros(keys, np.uint8),
                key_stamp=np.zeros(keys, np.int32), key_active=np.int32(0), key_rel=np.zeros(3), key_age=np.int32(0),
                key_misses=np.int32(0), step=np.int32(0), pose=np.asarray(pose, np.float64).copy())


def relative(pose, key):
    """The pose relative to the keyframe at `key`: (theta_k, u_kx, u_ky) of the N10 comment."""
    th = math.remainder(float(pose[2]) - float(key[2]), 2.0 * math.pi)
    dx, dy = pose[0] - key[0], pose[1] - key[1]
    c, s = np.cos(key[2]), np.sin(key[2])
    return np.array([th, c * dx + s * dy, (-s) * dx + c * dy])


def keyframe_map_oracle(r_cur, tab, state, person=None, max_range=20.0, window=16, gate=0.5, max_gap=0.3,
                        huber_delta=0.05, iters=16, eps_theta=1e-7, eps_u=1e-7, min_pivot=1e-6, key_dist=0.3, key_rot=0.3,
                        min_share=0.5, max_misses=2, revisit=0.5, sum=np.sum):
    """One step of pof_keyframe_map_match for one sensor in float64.  r_cur [N] float32, tab [3N], state: the dict of
    ``new_map_state`` (not modified; the ring size is its key_ranges'), person [N] bool: current points that do not
    vote.  -> (the state after the step, dict of the outputs of ``keyframe_oracle`` plus key_switched, key_slot)."""
    r1 = np.asarray(r_cur, np.float32)
    N = len(r1)
    K = len(state["key_valid"])
    tab = np.asarray(tab, np.float64)
    cs, sn = tab[N::2], tab[N + 1::2]
    phi0, dphi = tab[0], (tab[1] - tab[0] if N > 1 else 0.0)
    a = min(max(int(state["key_active"]), 0), K - 1)
    r0 = np.asarray(state["key_ranges"][a], np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v0 = np.isfinite(r0) & (r0.astype(np.float64) < max_range)
        valid = np.isfinite(r1) & (r1.astype(np.float64) < max_range)
        ax, ay = np.where(v0, r0.astype(np.float64) * cs, np.nan), np.where(v0, r0.astype(np.float64) * sn, np.nan)
        px, py = r1.astype(np.float64) * cs, r1.astype(np.float64) * sn
    if person is not None:
        valid = valid & ~np.asarray(person, bool)
    gated = np.where(valid, r1, np.float32(np.nan)).astype(np.float32)
    votes = int(valid.sum())
    margins = _Margins()
    old = np.asarray(state["pose"], np.float64)
    new = {k: np.copy(v) for k, v in state.items()}
    nan3 = np.full(3, np.nan)
    out = dict(motion=nan3, ok=np.uint8(0), count=np.int32(0), rms=np.nan, iters_used=np.int32(0), obs=0.0,
               corr=np.full(N, -1, np.int32), flow_residual=np.full((N, 2), np.nan))
    pose = old.copy()
    store, switched, slot, rel_new = False, False, a, None
    if not state["key_valid"][a]:
        store, age, misses = True, 0, 0
    else:
        init = np.asarray(state["key_rel"], np.float64)
        if not np.isfinite(init).all():
            init = np.zeros(3)
        failed, rel, count, rms, used, obs, corr, res = _iterate(ax, ay, px, py, valid, init, _centres(phi0, dphi, N),
                                                                 window, gate, max_gap, huber_delta, iters, eps_theta,
                                                                 eps_u, min_pivot, sum, margins)
        out.update(count=np.int32(count), iters_used=np.int32(used), obs=float(obs), corr=corr, flow_residual=res)
        if not failed:
            out.update(motion=rel, ok=np.uint8(1), rms=float(rms))
            pose = compose(np.asarray(state["key_pose"][a], np.float64), rel)
            u2, d2 = rel[1] * rel[1] + rel[2] * rel[2], key_dist * key_dist
            share = min_share * float(votes)
            margins.take("key_rot", [abs(abs(rel[0]) - key_rot)])
            margins.take("key_dist", [abs(u2 - d2)])
            margins.take("min_share", [abs(float(count) - share)])
            left = bool(abs(rel[0]) > key_rot or u2 > d2)
            stale = bool(float(count) < share)
            age, misses = (0 if left or stale else int(state["key_age"]) + 1), 0
            rel_new = rel.copy()
            if left:
                rev_rot, rev_d2 = revisit * key_rot, (revisit * key_dist) * (revisit * key_dist)
                win, win_d2 = -1, 0.0
                for k in range(K):
                    if k == a or not state["key_valid"][k]:
                        continue
                    cand = relative(pose, np.asarray(state["key_pose"][k], np.float64))
                    c2 = cand[1] * cand[1] + cand[2] * cand[2]
                    margins.take("revisit_rot", [abs(abs(cand[0]) - rev_rot)])
                    margins.take("revisit_dist", [abs(c2 - rev_d2)])
                    if abs(cand[0]) <= rev_rot and c2 <= rev_d2:
                        if win >= 0:
                            margins.take("winner", [abs(c2 - win_d2)])
                        if win < 0 or c2 < win_d2:
                            win, win_d2, rel_new = k, c2, cand
                if win >= 0:
                    switched, slot = True, win
                else:
                    store = True
                    free = [k for k in range(K) if not state["key_valid"][k]]
                    others = [k for k in range(K) if k != a and state["key_valid"][k]]
                    if free:
                        slot = free[0]
                    elif others:                               # the stamps are integers: the comparison is exact
                        slot = min(others, key=lambda k: (int(state["key_stamp"][k]), k))
            elif stale:
                store = True
        else:
            store = int(state["key_misses"]) + 1 > max_misses
            age = 0 if store else int(state["key_age"]) + 1
            misses = 0 if store else int(state["key_misses"]) + 1
    if store:
        new["key_ranges"][slot] = gated
        new["key_pose"][slot] = pose
        new["key_valid"][slot] = 1
        new["key_rel"] = np.zeros(3)
    elif rel_new is not None:
        new["key_rel"] = rel_new.copy()
    new["key_stamp"][slot] = state["step"]
    new.update(key_active=np.int32(slot), key_age=np.int32(age), key_misses=np.int32(misses),
               step=np.int32(int(state["step"]) + 1), pose=pose.copy())
    c1, s1 = np.cos(pose[2]), np.sin(pose[2])
    good = bool(out["ok"])
    out.update(key_replaced=np.uint8(store), key_switched=np.uint8(switched), key_slot=np.int32(slot),
               rot=np.array([c1, -s1, s1, c1]).astype(np.float32), trans=pose[:2].copy(),
               flow_trans=(pose[:2] - old[:2]) if good else np.zeros(2), margins=margins)
    return new, out


OUT_FLOATS, OUT_EXACT = ("motion", "rms", "obs", "flow_residual", "rot", "trans", "flow_trans"), \
    ("count", "ok", "iters_used", "key_replaced", "key_switched", "key_slot", "corr")
STATE_FLOATS = ("key_pose", "key_rel", "pose")
STATE_EXACT = ("key_valid", "key_stamp", "key_active", "key_age", "key_misses", "step", "key_ranges")


def run_map(scans, tab, pose0, keys, persons=None, state=None, sum=np.sum, **kw):
    """The steps of one sensor over scans [T,N] from ``new_map_state`` (or `state`) -> [(state after, outputs)]."""
    state = new_map_state(scans.shape[1], keys, pose0) if state is None else state
    steps = []
    for t in range(len(scans)):
        state, out = keyframe_map_oracle(scans[t], tab, state, person=None if persons is None else persons[t], sum=sum,
                                         **kw)
        steps.append((state, out))
    return steps


def map_tolerance(cases):
    """``sequence_tolerance`` of tests/test_keyframe.py for the map: `cases` = [(args, kwargs) of run_map] -> (TOL,
    the pairwise results).  100 x the largest disagreement of the pairwise and the sequential evaluation in any float
    of any step, at least 1e-13, never above 1e-10; everything exact agrees and every decision margin is >=
    MARGIN_MIN."""
    worst, results, smallest, decisions = 0.0, [], {}, 0
    for args, kw in cases:
        a, b = run_map(*args, **kw), run_map(*args, sum=seq_sum, **kw)
        for (sa, oa), (sb, ob) in zip(a, b):
            for got, want, exact, floats in ((oa, ob, OUT_EXACT, OUT_FLOATS), (sa, sb, STATE_EXACT, STATE_FLOATS)):
                for key in exact:
                    assert np.array_equal(got[key], want[key], equal_nan=True), key
                for key in floats:
                    x, y = np.asarray(got[key], np.float64), np.asarray(want[key], np.float64)
                    assert np.array_equal(np.isfinite(x), np.isfinite(y)), key
                    both = np.isfinite(x)
                    worst = max(worst, np.abs(x[both] - y[both]).max(initial=0.0))
            for kind, v in oa["margins"].items():
                if kind == "decisions":
                    decisions += v
                else:
                    smallest[kind] = min(smallest.get(kind, np.inf), v)
        results.append(a)
    tol = max(1e-13, 100.0 * worst)
    print("pairwise against sequential: %.3e -> TOL %.3e; %d decisions, smallest margins %s"
          % (worst, tol, decisions, {k: "%.2e" % v for k, v in sorted(smallest.items())}))
    assert tol <= 1e-10
    assert all(v >= MARGIN_MIN for v in smallest.values()), smallest
    return tol, results


def assert_map_step_matches(got, want, tol, what=""):
    """Device outputs and state of one sensor after one step (one dict of arrays) against the oracle's (state,
    outputs): everything discrete and every stored keyframe row bitwise, the rest within tol, NaN where the oracle
    has NaN."""
    for ref, exact, floats in ((want[1], OUT_EXACT, OUT_FLOATS), (want[0], STATE_EXACT, STATE_FLOATS)):
        for key in exact:
            x, y = np.asarray(got[key]), np.asarray(ref[key])
            assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True), (what, key, x, y)
        for key in floats:
            if key not in got:                                 # the pose terms, where the caller keeps none
                continue
            x, y = np.asarray(got[key], np.float64).reshape(-1), np.asarray(ref[key], np.float64).reshape(-1)
            assert np.array_equal(np.isnan(x), np.isnan(y)), (what, key)
            fin = np.isfinite(y)
            err = np.abs(x[fin] - y[fin]).max(initial=0.0)
            assert err <= tol, (what, key, err, tol)


# ---------------------------------------------------------------- scenes: paths that come back
def path_scans(seed, poses_of, N=450, noise=0.01, angle_inc=np.radians(0.5), people=False):
    """A seeded ``make_room`` room seen from the poses poses_of(rng) [T,3] (around the room's clear middle) ->
    (scans float32 [T,N], poses, gate or None as ``sequence`` of tests/test_keyframe.py, the room's segments)."""
    rng = np.random.default_rng(seed)
    phi = R.laser_phi(angle_inc, N)
    segs = make_room(rng)
    poses = poses_of(rng)
    scans = np.stack([(ray_cast(segs, p, phi) + rng.normal(0, 1.0, N) * noise).astype(np.float32) for p in poses])
    if not people:
        return scans, poses, None, segs
    got = [add_people(s, rng) for s in scans]
    scans = np.stack([g[0] for g in got])
    inst, num, cls = np.stack([g[1] for g in got]), np.array([g[2] for g in got], np.int32), np.stack([g[3] for g in got])
    return scans, poses, (inst, num, cls, np.stack([person_points(inst[t], num[t], cls[t]) for t in range(len(scans))])), segs


def line_poses(offsets, jitter=0.0):
    """Poses at `offsets` -- [T] distances along a seeded direction through the room's middle, or [T,3] rows (along,
    across, heading offset) in that frame -- the sensor looking along a fixed seeded direction; `jitter`: seeded
    sideways and heading noise."""
    off = np.asarray(offsets, np.float64)
    off = np.stack([off, np.zeros_like(off), np.zeros_like(off)], axis=1) if off.ndim == 1 else off

    def poses_of(rng):
        heading, look = rng.uniform(-np.pi, np.pi, 2)
        along, across = np.array([np.cos(heading), np.sin(heading)]), np.array([-np.sin(heading), np.cos(heading)])
        start = rng.uniform(-0.1, 0.1, 2) - 0.5 * off[:, 0].max() * along
        poses = np.zeros((len(off), 3))
        for t, (d, e, turn) in enumerate(off):
            poses[t, :2] = start + d * along + (e + rng.uniform(-jitter, jitter)) * across
            poses[t, 2] = look + turn + 2.0 * rng.uniform(-jitter, jitter)
        return poses
    return poses_of


def via(*points, step=0.11):
    """The way points (distances, or (along, across[, heading]) rows) joined by straight legs of equal steps of at
    most `step` metres -> [T,3] offsets for ``line_poses``."""
    pts = [np.concatenate([np.atleast_1d(np.asarray(p, np.float64)), np.zeros(3)])[:3] for p in points]
    rows = [pts[0]]
    for p, q in zip(pts[:-1], pts[1:]):
        n = max(1, int(np.ceil(np.hypot(*(q - p)[:2]) / step - 1e-9)))
        rows += [p + (q - p) * k / n for k in range(1, n + 1)]
    return np.stack(rows)


STEP, REACH, REST = 0.04, 30, 3
# out 1.2 m in 0.04 m steps and back the same way, then REST scans standing where the path began
OUT_AND_BACK = [STEP * k for k in range(REACH + 1)] + [STEP * k for k in range(REACH - 1, -1, -1)] + [0.0] * REST
LAP, RADIUS = 56, 0.4


def loop_poses(rng):
    """Two laps of a circle of radius 0.4 m around the room's middle, 56 scans each, the heading swaying +-0.2 rad
    with the lap, then REST scans standing where the path began."""
    look, phase = rng.uniform(-np.pi, np.pi, 2)
    centre = rng.uniform(-0.1, 0.1, 2)
    ang = phase + 2.0 * np.pi * np.concatenate([np.arange(2 * LAP + 1), np.full(REST, 2 * LAP)]) / LAP
    return np.stack([centre[0] + RADIUS * np.cos(ang), centre[1] + RADIUS * np.sin(ang),
                     look + 0.2 * np.sin(ang - phase)], axis=1)


PATHS = {"out_and_back": (line_poses(OUT_AND_BACK), REACH), "loop": (loop_poses, LAP)}
# the first six of the twelve seeds tried per path (401..412, 501..512); all twelve satisfy the test
PATH_SEEDS = {"out_and_back": (401, 402, 403, 404, 405, 406), "loop": (501, 502, 503, 504, 505, 506)}
_RETURN = {}


def position_errors(steps, poses):
    est = np.stack([s["pose"] for s, _ in steps])
    return np.hypot(est[:, 0] - poses[:, 0], est[:, 1] - poses[:, 1])


def return_row(name, seed):
    """-> dict of the figures of one path and seed: the map's and N9's (one slot) end error and largest error, the
    largest error of N9 standing still for 60 scans at the path's start in the same room, N9's replacements, the
    map's switches and the keyframes the map stored on the way back."""
    if (name, seed) not in _RETURN:
        poses_of, turn = PATHS[name]
        scans, poses, _, segs = path_scans(seed, poses_of)
        many = run_map(scans, TAB, poses[0], 16, **MAP)
        one = run_map(scans, TAB, poses[0], 1, **MAP)
        rng = np.random.default_rng(seed + 1000)
        phi = R.laser_phi(np.radians(0.5), 450)
        wall = ray_cast(segs, poses[0], phi)
        still = np.stack([(wall + rng.normal(0, 1.0, 450) * 0.01).astype(np.float32) for _ in range(60)])
        rest = run_map(still, TAB, poses[0], 1, **MAP)
        e_many, e_one = position_errors(many, poses), position_errors(one, poses)
        _RETURN[name, seed] = dict(
            map_end=e_many[-1], map_max=e_many.max(), n9_end=e_one[-1], n9_max=e_one.max(),
            still=position_errors(rest, np.repeat(poses[:1], 60, axis=0)).max(),
            n9_replaced=sum(int(o["key_replaced"]) for _, o in one[1:]),
            stored_out=sum(int(o["key_replaced"]) for _, o in many[1:turn + 1]),
            stored_back=sum(int(o["key_replaced"]) for _, o in many[turn + 1:]),
            switches=sum(int(o["key_switched"]) for _, o in many), ok=all(o["ok"] for _, o in many[1:] + one[1:]),
            last_slot=int(many[-1][1]["key_slot"]))
    return _RETURN[name, seed]


# ---------------------------------------------------------------- tests (no GPU): one slot is N9
@pytest.mark.parametrize("name", ["still", "sway", "walk"])
def test_one_slot_has_the_bits_of_the_keyframe_matcher(name):
    for seed in SEEDS[:3]:
        scans, poses, _ = scenario(name, seed)
        ring, single = new_map_state(450, 1, poses[0]), new_state(450, poses[0])
        replaced = 0
        for t in range(len(scans)):
            ring, got = keyframe_map_oracle(scans[t], TAB, ring, **MAP)
            single, want = keyframe_oracle(scans[t], TAB, single, **SETTINGS)
            for k in want:
                if k != "margins":
                    assert np.array_equal(got[k], want[k], equal_nan=True), (name, seed, t, k)
            for k in ("key_pose", "key_rel", "pose", "key_age", "key_misses"):
                assert np.array_equal(np.asarray(ring[k]).reshape(-1), np.asarray(single[k]).reshape(-1)), (name, seed, t, k)
            assert np.array_equal(ring["key_ranges"][0], single["key_ranges"], equal_nan=True)
            assert ring["key_valid"][0] == single["key_valid"] == 1
            assert got["key_slot"] == 0 and got["key_switched"] == 0 and ring["key_active"] == 0
            assert ring["step"] == t + 1 and ring["key_stamp"][0] == t
            replaced += int(got["key_replaced"]) if t else 0
        assert replaced >= 1 or name != "walk"


def test_one_slot_has_the_bits_of_the_keyframe_matcher_when_matches_fail():
    c0, c1 = corridor()
    pose0 = np.array([1.0, 2.0, 0.5])
    ring, single = new_map_state(450, 1, pose0), new_state(450, pose0)
    for t, scan in enumerate([c0, c1, c1, c1]):
        ring, got = keyframe_map_oracle(scan, TAB, ring, **dict(MAP, max_misses=1))
        single, want = keyframe_oracle(scan, TAB, single, **dict(SETTINGS, max_misses=1))
        for k in want:
            if k != "margins":
                assert np.array_equal(got[k], want[k], equal_nan=True), (t, k)
        for k in ("key_pose", "key_rel", "pose", "key_age", "key_misses"):
            assert np.array_equal(np.asarray(ring[k]).reshape(-1), np.asarray(single[k]).reshape(-1)), (t, k)
        assert np.array_equal(ring["key_ranges"][0], single["key_ranges"], equal_nan=True)


# ---------------------------------------------------------------- policy: every branch, the state field by field
def _state_is(state, **want):
    for k, v in want.items():
        assert np.array_equal(np.asarray(state[k]), np.asarray(v), equal_nan=True), (k, state[k], v)


def _line(seed, offsets, keys, **kw):
    scans, poses, _, _ = path_scans(seed, line_poses(offsets))
    return scans, poses, run_map(scans, TAB, poses[0], keys, **dict(MAP, **kw))


def _events(steps, key):
    return [t for t, (_, o) in enumerate(steps) if o[key]]


def _dist(state, k):
    return float(np.hypot(*relative(state["pose"], state["key_pose"][k])[1:]))


def test_seeding_takes_the_active_slot():
    scans, poses, _ = sequence(1, 201)
    scans[0, 5], scans[0, 9] = 25.0, np.inf
    start = new_map_state(450, 3, poses[0])
    start["key_active"] = np.int32(2)
    state, out = keyframe_map_oracle(scans[0], TAB, start, **MAP)
    want = scans[0].copy()
    want[[5, 9]] = np.nan
    _state_is(state, key_valid=[0, 0, 1], key_active=2, key_stamp=[0, 0, 0], step=1, key_rel=np.zeros(3), key_age=0,
              key_misses=0, pose=poses[0])
    assert np.array_equal(state["key_ranges"][2], want, equal_nan=True) and not state["key_ranges"][:2].any()
    assert np.array_equal(state["key_pose"][2], poses[0]) and not state["key_pose"][:2].any()
    assert out["ok"] == 0 and np.isnan(out["motion"]).all() and np.isnan(out["rms"]) and out["count"] == 0
    assert out["iters_used"] == 0 and out["obs"] == 0.0 and out["key_replaced"] == 1 and out["key_switched"] == 0
    assert out["key_slot"] == 2 and (out["corr"] == -1).all() and np.isnan(out["flow_residual"]).all()
    assert np.array_equal(out["trans"], poses[0][:2]) and np.array_equal(out["flow_trans"], np.zeros(2))
    _state_is(start, key_valid=[0, 0, 0], step=0)               # the oracle works on a copy


def test_holding_and_a_new_keyframe_into_the_first_free_slot():
    scans, poses, steps = _line(211, via(0.0, 0.44), 3)        # 0.11 m per scan
    for t in (1, 2):
        s, o = steps[t]
        assert o["ok"] and not o["key_replaced"] and not o["key_switched"] and o["key_slot"] == 0
        _state_is(s, key_active=0, key_age=t, key_misses=0, key_valid=[1, 0, 0], key_rel=o["motion"], step=t + 1,
                  key_stamp=[t, 0, 0], key_ranges=steps[0][0]["key_ranges"], key_pose=steps[0][0]["key_pose"])
    s, o = steps[3]                                            # 0.33 m from slot 0
    assert o["ok"] and np.hypot(*o["motion"][1:]) > 0.3 and o["key_replaced"] and not o["key_switched"] and o["key_slot"] == 1
    _state_is(s, key_active=1, key_age=0, key_misses=0, key_valid=[1, 1, 0], key_rel=np.zeros(3), step=4,
              key_stamp=[2, 3, 0])
    assert np.array_equal(s["pose"], compose(steps[0][0]["key_pose"][0], o["motion"]))
    assert np.array_equal(s["key_pose"][1], s["pose"]) and np.array_equal(s["key_pose"][0], poses[0])
    assert np.array_equal(s["key_ranges"][1], scans[3]) and np.array_equal(s["key_ranges"][0], scans[0])
    assert not s["key_ranges"][2].any()
    s, o = steps[4]                                            # matched against slot 1, from rest
    assert o["ok"] and np.hypot(*o["motion"][1:]) < 0.15 and s["key_age"] == 1 and s["key_active"] == 1
    assert np.array_equal(s["pose"], compose(steps[3][0]["key_pose"][1], o["motion"]))


def test_eviction_takes_the_least_recently_active_slot_and_never_the_active_one():
    scans, poses, steps = _line(212, via(0.0, 1.32), 3)        # a keyframe every third scan
    assert _events(steps, "key_replaced") == [0, 3, 6, 9, 12] and not _events(steps, "key_switched")
    assert [int(steps[t][1]["key_slot"]) for t in (0, 3, 6, 9, 12)] == [0, 1, 2, 0, 1]     # full, then slot 0, then 1
    _state_is(steps[8][0], key_valid=[1, 1, 1], key_stamp=[2, 5, 8], key_active=2)
    _state_is(steps[9][0], key_stamp=[9, 5, 8], key_active=0)
    assert np.array_equal(steps[9][0]["key_ranges"][0], scans[9]) and np.array_equal(steps[9][0]["key_pose"][0], steps[9][0]["pose"])
    assert np.array_equal(steps[9][0]["key_ranges"][1:], steps[8][0]["key_ranges"][1:])
    _state_is(steps[12][0], key_stamp=[11, 12, 8], key_active=1)
    # a tie of the stamps goes to the lower index, and the active slot is not the victim even with the smallest stamp
    tied = {k: np.copy(v) for k, v in steps[8][0].items()}
    tied["key_stamp"] = np.array([5, 5, 0], np.int32)          # slot 2 is active
    s, o = keyframe_map_oracle(scans[9], TAB, tied, **MAP)
    assert o["key_replaced"] and o["key_slot"] == 0 and s["key_stamp"][0] == 9
    tied["key_stamp"] = np.array([7, 5, 0], np.int32)
    s, o = keyframe_map_oracle(scans[9], TAB, tied, **MAP)
    assert o["key_replaced"] and o["key_slot"] == 1
    # one slot: the active one is all there is
    one = run_map(scans[:4], TAB, poses[0], 1, **MAP)
    assert one[3][1]["key_replaced"] and one[3][1]["key_slot"] == 0 and np.array_equal(one[3][0]["key_ranges"][0], scans[3])


def test_a_return_switches_and_the_next_match_is_anchored_on_the_old_keyframe():
    scans, poses, steps = _line(213, via(0.0, 0.33, 0.02, 0.04), 4)
    assert _events(steps, "key_replaced") == [0, 3] and _events(steps, "key_switched") == [6]
    s1, (s2, o2), (s3, o3) = steps[5][0], steps[6], steps[7]
    # 0.31 m back from slot 1, 0.02 m from slot 0: a switch, nothing stored, the pose is the one formed from slot 1
    assert o2["ok"] and not o2["key_replaced"] and o2["key_slot"] == 0 and np.hypot(*o2["motion"][1:]) > 0.3
    pose2 = compose(s1["key_pose"][1], o2["motion"])
    _state_is(s2, key_active=0, key_age=0, key_misses=0, key_valid=[1, 1, 0, 0], key_stamp=[6, 5, 0, 0], step=7,
              pose=pose2, key_ranges=s1["key_ranges"], key_pose=s1["key_pose"], key_rel=relative(pose2, s1["key_pose"][0]))
    assert np.hypot(*s2["key_rel"][1:]) < 0.03 and (o2["corr"] >= 0).sum() > 300
    # the next scan: matched against slot 0 from that key_rel, pose = key_pose[0] o match -- the way round is dropped
    assert o3["ok"] and not o3["key_switched"] and not o3["key_replaced"] and o3["key_slot"] == 0
    _state_is(s3, pose=compose(poses[0], o3["motion"]), key_age=1, key_active=0, key_rel=o3["motion"])
    assert np.array_equal(s3["key_pose"][0], poses[0])


def test_no_switch_inside_key_dist_but_outside_the_revisit_radius():
    # slot 1 at (0.33, 0); at (0.05, 0.22) the sensor is 0.36 m from it and 0.23 m from slot 0: inside key_dist = 0.3,
    # outside revisit * key_dist = 0.15
    scans, poses, steps = _line(214, via(0.0, 0.33, (0.05, 0.22)), 4)
    assert _events(steps, "key_replaced") == [0, 3, 7] and not _events(steps, "key_switched")
    s, o = steps[7]
    assert o["ok"] and o["key_slot"] == 2 and 0.15 < _dist(s, 0) < 0.3 and abs(relative(s["pose"], s["key_pose"][0])[0]) < 0.15
    _state_is(s, key_valid=[1, 1, 1, 0], key_active=2, key_rel=np.zeros(3))
    # revisit = 1 takes it, revisit = 0 takes nothing at all
    s, o = keyframe_map_oracle(scans[7], TAB, steps[6][0], **dict(MAP, revisit=1.0))
    assert o["key_switched"] and not o["key_replaced"] and o["key_slot"] == 0
    scans, poses, steps = _line(213, via(0.0, 0.33, 0.02), 4, revisit=0.0)
    assert steps[6][1]["key_replaced"] and not steps[6][1]["key_switched"] and steps[6][1]["key_slot"] == 2
    # the heading alone keeps a candidate out: back at slot 0's place but turned by 0.2 rad > revisit * key_rot
    scans, poses, steps = _line(213, via(0.0, 0.33, (0.02, 0.0, 0.2)), 4)
    s, o = steps[6]
    assert o["ok"] and o["key_replaced"] and not o["key_switched"] and o["key_slot"] == 2
    assert _dist(s, 0) < 0.03 and 0.15 < abs(relative(s["pose"], s["key_pose"][0])[0]) < 0.3


def test_the_nearer_of_two_qualifying_keyframes_wins():
    # slot 0 at (0, 0), slot 1 at (0.33, 0), slot 2 on the way to (0.2, 0.45); back down to (0.2, 0.05): 0.31 m from
    # slot 2, 0.21 m from slot 0 and 0.14 m from slot 1, both inside revisit * key_dist = 0.24
    scans, poses, steps = _line(215, via(0.0, 0.33, (0.2, 0.45), (0.2, 0.05)), 4, revisit=0.8)
    stored, switched = _events(steps, "key_replaced"), _events(steps, "key_switched")
    assert len(stored) == 3 and switched == [len(steps) - 1]
    s, o = steps[-1]
    assert _dist(s, 1) < _dist(s, 0) <= 0.24 and _dist(s, 2) > 0.3 and o["key_slot"] == 1 and not o["key_replaced"]
    assert np.array_equal(s["key_rel"], relative(s["pose"], s["key_pose"][1]))
    # an exact tie goes to the lower slot: slot 1 given the pose of slot 0
    tie = {k: np.copy(v) for k, v in steps[-2][0].items()}
    tie["key_pose"][1] = tie["key_pose"][0]
    s, o = keyframe_map_oracle(scans[-1], TAB, tie, **dict(MAP, revisit=0.8))
    assert o["key_switched"] and o["key_slot"] == 0


def _changed_scene(seed, offsets):
    scans, poses, _, _ = path_scans(seed, line_poses(offsets))
    changed = scans[-1].copy()
    changed[:250] = np.maximum(changed[:250] - 2.0, 0.3)       # something large moved in front of 250 beams
    return np.concatenate([scans[:-1], changed[None]]), poses


def test_stale_only_overwrites_the_active_slot_in_place():
    scans, poses = _changed_scene(216, via(0.0, 0.33, 0.34, 0.35))
    steps = run_map(scans, TAB, poses[0], 4, **MAP)
    assert _events(steps, "key_replaced") == [0, 3, 5] and not _events(steps, "key_switched")
    (s2, o2), (s3, o3) = steps[4], steps[5]
    assert o2["key_slot"] == 1 and o3["ok"] and o3["key_slot"] == 1
    assert 3 <= o3["count"] < 0.5 * 450 and np.hypot(*o3["motion"][1:]) < 0.3 and abs(o3["motion"][0]) < 0.3
    _state_is(s3, key_valid=[1, 1, 0, 0], key_active=1, key_age=0, key_rel=np.zeros(3), key_stamp=[2, 5, 0, 0],
              pose=compose(s2["key_pose"][1], o3["motion"]))
    assert np.array_equal(s3["key_ranges"][1], scans[5]) and np.array_equal(s3["key_pose"][1], s3["pose"])
    assert np.array_equal(s3["key_ranges"][0], scans[0]) and not s3["key_ranges"][2:].any()


def test_left_and_stale_together_take_the_left_path():
    scans, poses = _changed_scene(217, via(0.0, 0.33, 0.02))
    steps = run_map(scans, TAB, poses[0], 4, **MAP)
    s, o = steps[6]
    assert o["ok"] and 3 <= o["count"] < 0.5 * 450 and np.hypot(*o["motion"][1:]) > 0.3   # left and stale
    assert o["key_switched"] and not o["key_replaced"] and o["key_slot"] == 0             # ... and back at slot 0
    assert np.array_equal(s["key_ranges"], steps[5][0]["key_ranges"], equal_nan=True)


def test_a_failed_match_after_a_switch_leaves_the_pose_and_max_misses_re_anchors_the_active_slot_only():
    c0, c1 = corridor()
    scans, poses, steps = _line(213, via(0.0, 0.33, 0.02), 4, max_misses=1)
    state = steps[6][0]                                        # switched to slot 0
    assert steps[6][1]["key_switched"] and state["step"] == 7
    state = dict(state, key_ranges=np.stack([c0] + list(state["key_ranges"][1:])))
    s, o = keyframe_map_oracle(c1, TAB, state, **dict(MAP, max_misses=1))
    assert o["ok"] == 0 and np.isnan(o["motion"]).all() and o["key_replaced"] == 0 and o["key_switched"] == 0
    _state_is(s, pose=state["pose"], key_rel=state["key_rel"], key_pose=state["key_pose"], key_active=0, key_age=1,
              key_misses=1, key_stamp=[7, 5, 0, 0], step=8, key_ranges=state["key_ranges"])
    s2, o2 = keyframe_map_oracle(c1, TAB, s, **dict(MAP, max_misses=1))
    assert o2["ok"] == 0 and o2["key_replaced"] == 1 and o2["key_switched"] == 0 and o2["key_slot"] == 0
    _state_is(s2, pose=state["pose"], key_rel=np.zeros(3), key_active=0, key_age=0, key_misses=0, key_valid=[1, 1, 0, 0])
    assert np.array_equal(s2["key_pose"][0], state["pose"]) and np.array_equal(s2["key_pose"][1:], state["key_pose"][1:])
    assert np.array_equal(s2["key_ranges"][0], np.where(c1 < 20.0, c1, np.float32(np.nan)), equal_nan=True)
    assert np.array_equal(s2["key_ranges"][1:], state["key_ranges"][1:])


def test_a_heading_difference_across_pi_uses_the_remainder():
    assert abs(relative(np.array([0.0, 0.0, 3.1]), np.array([0.0, 0.0, -3.1]))[0] - (6.2 - 2 * np.pi)) < 1e-15
    assert abs(relative(np.array([0.0, 0.0, -3.1]), np.array([0.0, 0.0, 3.1]))[0] + (6.2 - 2 * np.pi)) < 1e-15
    # slot 0 is revisited with its heading written on the other side of -pi: phi - phi_k is 2 pi + 0.04
    scans, poses, _, _ = path_scans(218, lambda rng: np.array([[0.0, 0.0, np.pi - 0.02]]) + via(0.0, 0.33, (0.02, 0.0, 0.04)))
    steps = run_map(scans, TAB, poses[0], 4, **MAP)
    assert _events(steps, "key_switched") == [6]
    wrapped = {k: np.copy(v) for k, v in steps[5][0].items()}
    wrapped["key_pose"][0, 2] -= 2 * np.pi
    s, o = keyframe_map_oracle(scans[6], TAB, wrapped, **MAP)
    assert o["key_switched"] and o["key_slot"] == 0 and abs(s["key_rel"][0] - 0.04) < 5e-3
    assert abs(s["pose"][2] - wrapped["key_pose"][0, 2]) > 6.0
    assert np.abs(s["key_rel"][1:] - steps[6][0]["key_rel"][1:]).max() < 1e-12


def test_people_are_stored_as_nan_in_whichever_slot_is_written():
    scans, poses, gate, _ = path_scans(219, line_poses(via(0.0, 0.66)), people=True)
    person = gate[3]
    steps = run_map(scans, TAB, poses[0], 2, persons=person, **MAP)
    stored = _events(steps, "key_replaced")
    assert stored == [0, 3, 6] and [int(steps[t][1]["key_slot"]) for t in stored] == [0, 1, 0]
    for t, slot in zip(stored, (0, 1, 0)):
        key = steps[t][0]["key_ranges"][slot]
        assert person[t].any() and np.isnan(key[person[t]]).all()
        assert np.array_equal(key[~person[t]], scans[t][~person[t]])
        assert (steps[t][1]["corr"][person[t]] == -1).all()


# ---------------------------------------------------------------- drift on a return
@pytest.mark.parametrize("name", sorted(PATHS))
def test_a_return_drops_the_drift_of_the_way_round(name):
    rows = [return_row(name, seed) for seed in PATH_SEEDS[name]]
    for seed, r in zip(PATH_SEEDS[name], rows):
        print("%s seed %d: end error map %.3e m, one slot %.3e m; largest map %.3e m, one slot %.3e m; standing still "
              "%.3e m; one slot replaced %d, the map stored %d out and %d back, switched %d times, ends on slot %d"
              % (name, seed, r["map_end"], r["n9_end"], r["map_max"], r["n9_max"], r["still"], r["n9_replaced"],
                 r["stored_out"], r["stored_back"], r["switches"], r["last_slot"]))
    for r in rows:
        assert r["ok"] and r["n9_replaced"] >= 4
        assert r["switches"] >= 1 and r["stored_back"] == 0 and r["last_slot"] == 0
        assert r["map_end"] < r["n9_end"]
        assert r["map_end"] < 2.0 * r["still"]


# ---------------------------------------------------------------- margins: the committed cases of the GPU tests
# N -> B, angle increment (degrees), range noise (m), window, seed: the shapes of tests/test_keyframe_gpu.py; the
# noise-free N = 4096 seed is the third tried (631 and 632 have a nearest-vertex margin below MARGIN_MIN)
SHAPES = {450: (3, 0.5, 0.01, 16, 601), 512: (2, 0.5, 0.01, 16, 611), 513: (2, 0.5, 0.01, 16, 621),
          4096: (1, 0.05, 0.0, 64, 633)}
T_GPU, KEYS_GPU, KEY_DIST_GPU = 10, 3, 0.08
VARIANTS = ("plain", "huber", "gated")
# 0.05 m per scan out to 0.3 m and back: slot 1 at 0.10, slot 2 at 0.20 (the ring is full), slot 0 evicted at 0.30,
# and at 0.20 on the way back, 0.10 m from there, a switch to slot 2
WALK_GPU = [0.0, 0.05, 0.10, 0.15, 0.20, 0.25, 0.30, 0.25, 0.20, 0.15]


def shape_case(N, variant, keys=KEYS_GPU):
    """-> (angle increment, scans [T,B,N], poses [T,B,3], gate per sensor or None, settings, keys)."""
    B, inc, noise, window, seed = SHAPES[N]
    seqs = [path_scans(seed + b, line_poses(WALK_GPU, jitter=0.004), N=N, noise=noise, angle_inc=np.radians(inc),
                       people=variant == "gated") for b in range(B)]
    kw = dict(MAP, window=window, key_dist=KEY_DIST_GPU)
    if variant == "plain":
        kw["huber_delta"] = 0.0
    return (np.radians(inc), np.stack([s[0] for s in seqs], axis=1), np.stack([s[1] for s in seqs], axis=1),
            [s[2] for s in seqs] if variant == "gated" else None, kw, keys)


def case_oracle(case):
    inc, scans, poses, gates, kw, keys = case
    tab = angle_table(scans.shape[2], inc)
    return map_tolerance([((scans[:, b], tab, poses[0, b], keys),
                           dict(kw, persons=None if gates is None else gates[b][3])) for b in range(scans.shape[1])])


def assert_fills_evicts_and_switches(steps):
    slots = [int(o["key_slot"]) for _, o in steps]
    stored = [t for t, (_, o) in enumerate(steps) if o["key_replaced"]]
    switched = [t for t, (_, o) in enumerate(steps) if o["key_switched"]]
    assert all(o["ok"] for _, o in steps[1:]), slots
    assert stored == [0, 2, 4, 6] and [slots[t] for t in stored] == [0, 1, 2, 0], (stored, slots)
    assert switched == [8] and slots[8] == 2 and slots[9] == 2, (switched, slots)


@pytest.mark.parametrize("N", sorted(SHAPES))
def test_summation_order_the_tolerance_rule_and_the_decision_margins(N):
    for variant in VARIANTS:
        tol, steps = case_oracle(shape_case(N, variant))
        for s in steps:
            assert_fills_evicts_and_switches(s)
            kinds = set().union(*(set(o["margins"]) for _, o in s))
            assert {"revisit_rot", "revisit_dist", "key_rot", "key_dist", "min_share", "centre"} <= kinds


def test_margins_with_sixty_four_slots_and_of_the_paths_that_return():
    tol, steps = case_oracle(shape_case(450, "huber", keys=64))
    assert [int(o["key_slot"]) for _, o in steps[0]] == [0, 0, 1, 1, 2, 2, 3, 3, 2, 2]
    assert steps[0][8][1]["key_switched"]
    for name in sorted(PATHS):
        scans, poses, _, _ = path_scans(PATH_SEEDS[name][0], PATHS[name][0])
        map_tolerance([((scans[:70], TAB, poses[0], 16), MAP)])
    # the winner against the runner-up: the sequence of test_the_nearer_of_two_qualifying_keyframes_wins
    scans, poses, _, _ = path_scans(215, line_poses(via(0.0, 0.33, (0.2, 0.45), (0.2, 0.05))))
    tol, (steps,) = map_tolerance([((scans, TAB, poses[0], 4), dict(MAP, revisit=0.8))])
    assert steps[-1][1]["key_switched"] and "winner" in steps[-1][1]["margins"]


def stream_case(B=2):
    """The streaming detector's sequence: B sensors on WALK_GPU with the settings of the GPU cases."""
    seqs = [path_scans(641 + b, line_poses(WALK_GPU, jitter=0.004)) for b in range(B)]
    return np.stack([s[0] for s in seqs], axis=1), np.stack([s[1] for s in seqs], axis=1)


def test_margins_of_the_streaming_case():
    scans, poses = stream_case()
    tol, steps = map_tolerance([((scans[:, b], TAB, poses[0, b], KEYS_GPU), dict(MAP, key_dist=KEY_DIST_GPU))
                                for b in range(scans.shape[1])])
    for s in steps:
        assert_fills_evicts_and_switches(s)


# ---------------------------------------------------------------- host side
def _raw_args(**kw):
    import ctypes
    one = ctypes.c_void_p(16)
    g = lambda k, d: kw.get(k, d)
    return [one, one, None, None, None, 0.5, 20.0, g("window", 16), g("gate", 0.5), g("max_gap", 0.3),
            g("huber_delta", 0.05), g("iters", 16), 1e-7, 1e-7, 1e-6, g("key_dist", 0.3), g("key_rot", 0.3),
            g("min_share", 0.5), g("max_misses", 2), g("revisit", 0.5), g("B", 1), g("N", 450), g("keys", 16)] \
        + [one] * 19 + [None] * 6


def test_abi_and_python_surface():
    import ctypes
    import os
    from planar_optical_flow_amd import _lib, build, ops
    build.build(verbose=False)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pof_abi.h")).read()
    assert "pof_keyframe_map_match" in _lib.SIGNATURES and "int pof_keyframe_map_match(" in header
    assert "N10 keyframe map" in header and "tests/test_keyframe_map.py" in header and "#define POF_ABI_VERSION 1" in header
    assert len(_lib.SIGNATURES["pof_keyframe_map_match"][1]) == 48
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "pof_keyframe_map_match") and hasattr(_lib.load(), "pof_keyframe_map_match")
    assert ops.KeyframeMapState._fields == ("key_ranges", "key_pose", "key_valid", "key_stamp", "key_active", "key_rel",
                                            "key_age", "key_misses", "step", "pose")
    assert ops.KeyframeMapMatch._fields == ("motion", "count", "rms", "ok", "iters_used", "obs", "key_replaced",
                                            "key_switched", "key_slot", "corr", "flow_residual")
    # the library's own argument checks, before any launch: no pointer is dereferenced
    lib = _lib.load()
    call = lambda a: lib.pof_keyframe_map_match(*a)
    for bad in (dict(window=0), dict(window=65), dict(iters=0), dict(iters=33), dict(gate=-1.0), dict(max_gap=-0.1),
                dict(huber_delta=-0.05), dict(gate=float("nan")), dict(B=-1), dict(N=0), dict(key_dist=-0.1),
                dict(key_rot=-0.1), dict(min_share=-0.5), dict(key_dist=float("nan")), dict(key_rot=float("nan")),
                dict(min_share=float("nan")), dict(max_misses=-1), dict(keys=0), dict(keys=65), dict(keys=-1),
                dict(revisit=-0.1), dict(revisit=1.5), dict(revisit=float("nan"))):
        assert call(_raw_args(**bad)) == _lib.POF_E_BADARG, bad
    assert call(_raw_args(N=4097)) == _lib.POF_E_SHAPE
    assert call(_raw_args(N=4097, keys=65)) == _lib.POF_E_BADARG
    for fine in (dict(B=0), dict(B=0, keys=1), dict(B=0, keys=64), dict(B=0, revisit=0.0), dict(B=0, revisit=1.0)):
        assert call(_raw_args(**fine)) == _lib.POF_OK, fine
    for missing in list(range(23, 42)):                        # every state and output pointer up to key_slot
        a = _raw_args()
        a[missing] = None
        assert call(a) == _lib.POF_E_BADARG, missing
    a = _raw_args()
    a[2] = ctypes.c_void_p(16)                                 # the instance mask without the other NMS results
    assert call(a) == _lib.POF_E_BADARG


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    import torch
    from planar_optical_flow_amd import ops
    B, N, K = 2, 8, 3
    cur, tab = torch.ones(B, N), torch.zeros(3 * N, dtype=torch.float64)
    state = ops.keyframe_map_buffers(B, N, K, "cpu")
    assert [tuple(t.shape) for t in state] == [(B, K, N), (B, K, 3), (B, K), (B, K), (B,), (B, 3), (B,), (B,), (B,), (B, 3)]
    assert [t.dtype for t in state] == [torch.float32, torch.float64, torch.uint8, torch.int32, torch.int32,
                                        torch.float64, torch.int32, torch.int32, torch.int32, torch.float64]
    out = ops.keyframe_map_match_buffers(B, N, "cpu")
    assert [tuple(t.shape) for t in out] == [(B, 3), (B,), (B,), (B,), (B,), (B,), (B,), (B,), (B,), (B, N), (B, N, 2)]
    assert out.key_switched.dtype == torch.uint8 and out.key_slot.dtype == torch.int32
    with pytest.raises(TypeError):
        ops.keyframe_map_match(cur, tab, state)
    for bad in (dict(window=0), dict(window=65), dict(iters=0), dict(iters=33), dict(gate=-0.5), dict(max_gap=-0.3),
                dict(huber_delta=-1.0), dict(gate=float("nan")), dict(key_dist=-0.3), dict(key_rot=float("nan")),
                dict(min_share=-0.1), dict(max_misses=-1), dict(revisit=-0.1), dict(revisit=1.01),
                dict(revisit=float("nan")),
                dict(instance_mask=torch.zeros(B, N, dtype=torch.int32), num_det=torch.zeros(B, dtype=torch.int32))):
        with pytest.raises(ValueError):
            ops.keyframe_map_match(cur, tab, state, **bad)
    for keys in (0, 65, -3):
        with pytest.raises(ValueError):
            ops.keyframe_map_buffers(B, N, keys, "cpu")
    sig = inspect.signature(ops.keyframe_map_match)
    assert list(sig.parameters) == ["ranges_cur", "tab", "state", "instance_mask", "num_det", "det_cls", "cls_thresh",
                                    "max_range", "window", "gate", "max_gap", "huber_delta", "iters", "eps_theta",
                                    "eps_u", "min_pivot", "key_dist", "key_rot", "min_share", "max_misses", "revisit",
                                    "out", "rot", "trans", "flow_trans"]
    assert {k: sig.parameters[k].default for k in MAP} == MAP
    assert all(p.kind is p.KEYWORD_ONLY for p in list(sig.parameters.values())[3:])
    assert list(inspect.signature(ops.keyframe_map_buffers).parameters) == ["B", "N", "keys", "device"]
    # keyframe_map_reset: tensor operations in place
    for t in state:
        t.fill_(3)
    ops.keyframe_map_reset(state, pose=[1.0, 2.0, 0.5])
    assert all(not t.any() for t in state[:9]) and torch.equal(state.pose, torch.tensor([[1.0, 2.0, 0.5]] * B, dtype=torch.float64))
    ops.keyframe_map_reset(state)
    assert not state.pose.any()


def test_utils_and_streaming_signatures():
    from planar_optical_flow_amd.src.utils import utils as u
    from planar_optical_flow_amd.streaming import StreamingDetector
    sig = inspect.signature(u.KeyframeMapOdometry.__init__)
    assert list(sig.parameters) == ["self", "scan_phi", "keys", "revisit", "kw"]
    assert sig.parameters["keys"].default == 16 and sig.parameters["revisit"].default == 0.5
    assert sig.parameters["kw"].kind is inspect.Parameter.VAR_KEYWORD
    assert list(inspect.signature(u.KeyframeMapOdometry.update).parameters) == ["self", "scan", "pred_cls", "pred_reg"]
    assert list(inspect.signature(u.KeyframeMapOdometry.reset).parameters) == ["self", "pose"]
    src = inspect.getsource(StreamingDetector)
    for word in ('"keyframe_map"', "keyframe_map_match", "keyframe_map_buffers", "keyframe_map_reset", "key_switched",
                 "key_slot"):
        assert word in src, word
    # the detector's defaults are no literals in its source any more: they are what it hands the stage
    from planar_optical_flow_amd.streaming import stage_settings
    kw = stage_settings("ego_motion", {}, 0.5, "keyframe_map")
    assert (kw["keys"], kw["revisit"]) == (16, 0.5)
