"""Keyframe scan matching (pof_keyframe_match, N9) without a GPU: ``keyframe_oracle`` is the float64 NumPy restatement
of the N9 comment in include/pof_abi.h for one sensor and one step on explicit state, built on the helpers of
tests/test_scan_match.py (only the window centre and the keyframe policy are new).  It is run here on seeded polygon
rooms next to scan-to-scan matching as the streaming detector runs it (every pair started from the previous motion), on
every branch of the policy, and under the summation-order / decision-margin rule of N8.
tests/test_keyframe_gpu.py imports the helpers below.

Bounds against the true pose (metres, the largest position error over a sequence): fixed from the restatement's own
results on the committed seeds (printed by the tests; the worst is quoted next to each constant) with a factor 2.
Device against oracle (``sequence_tolerance``): N8's rule -- 100 x the largest disagreement between the oracle's own
pairwise and sequential evaluations of the sequence at hand, at least 1e-13 and asserted to stay below 1e-10; every
discrete decision (N8's kinds, the rounding of every window centre, the three replacement tests) keeps a margin
>= MARGIN_MIN in every committed case."""
import inspect

import numpy as np
import pytest

from oracle import ref_numpy as R
from test_ego_motion import seq_sum
from test_scan_match import (DEFAULTS, MARGIN_MIN, _Margins, _iterate, add_people, angle_table, corridor, make_room,
                             match_oracle, person_points, ray_cast)

POLICY = dict(key_dist=0.3, key_rot=0.3, min_share=0.5, max_misses=2)
SETTINGS = dict(DEFAULTS, **POLICY)
# the largest position error of the restatement over a sequence, worst of the six committed seeds, times 2
BOUND_STILL = 2 * 5.68e-3           # keyframe 2.33e-3 to 5.68e-3 m; scan-to-scan 5.00e-3 to 3.97e-2 m; no key replaced
BOUND_SWAY = 2 * 5.35e-3            # keyframe 2.75e-3 to 5.35e-3 m; scan-to-scan 5.59e-3 to 1.72e-2 m; no key replaced
BOUND_WALK = 2 * 4.65e-3            # keyframe 2.75e-3 to 4.65e-3 m; scan-to-scan 3.70e-3 to 7.93e-3 m; 4 to 6 keys replaced
SEEDS = (101, 102, 103, 104, 105, 106)


# ---------------------------------------------------------------- the restatement: one sensor, one step
def new_state(N, pose=(0.0, 0.0, 0.0)):
    """The state of a sensor without a keyframe, as ops.keyframe_buffers / keyframe_reset leave it."""
    return dict(key_ranges=np.zeros(N, np.float32), key_pose=np.zeros(3), key_rel=np.zeros(3), key_valid=np.uint8(0),
                key_age=np.int32(0), key_misses=np.int32(0), pose=np.asarray(pose, np.float64).copy())


def compose(pose, rel):
    """key_pose o (theta, u) with pof_pose_advance's formulas."""
    c, s = np.cos(pose[2]), np.sin(pose[2])
    return np.array([pose[0] + (c * rel[1] - s * rel[2]), pose[1] + (s * rel[1] + c * rel[2]), pose[2] + rel[0]])


def _centres(phi0, dphi, N):
    """N9's window centres for ``_correspond`` of tests/test_scan_match.py: mid [N] int, the beam every transformed
    point falls on; the rounding margins of the points that vote."""
    def centres(qx, qy, th, valid, margins):
        if dphi == 0.0:
            return np.zeros(len(qx), np.int64)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            qd = (np.arctan2(qy, qx) - phi0) / dphi
            t = np.rint(qd)
        t = np.where(t >= -N, t, -N)                           # a NaN gives -N
        t = np.where(t <= 2 * N, t, 2 * N)
        fin = valid & np.isfinite(qd)
        margins.take("centre", np.abs(np.abs(qd[fin] - np.floor(qd[fin])) - 0.5))
        return t.astype(np.int64)
    return centres


def keyframe_oracle(r_cur, tab, state, person=None, max_range=20.0, window=16, gate=0.5, max_gap=0.3, huber_delta=0.05,
                    iters=16, eps_theta=1e-7, eps_u=1e-7, min_pivot=1e-6, key_dist=0.3, key_rot=0.3, min_share=0.5,
                    max_misses=2, sum=np.sum):
    """One step of pof_keyframe_match for one sensor in float64.  r_cur [N] float32, tab [3N], state: the dict of
    ``new_state`` (not modified), person [N] bool: current points that do not vote.  -> (the state after the step, dict
    of motion [3], ok, count, rms, iters_used, obs, key_replaced, corr [N], flow_residual [N,2], rot [4] float32, trans
    [2], flow_trans [2], and margins: the smallest margin of every kind of discrete decision, and their number)."""
    r1 = np.asarray(r_cur, np.float32)
    N = len(r1)
    tab = np.asarray(tab, np.float64)
    cs, sn = tab[N::2], tab[N + 1::2]
    phi0, dphi = tab[0], (tab[1] - tab[0] if N > 1 else 0.0)
    r0 = np.asarray(state["key_ranges"], np.float32)
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
    if not state["key_valid"]:
        replace, age, misses = True, 0, 0
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
            pose = compose(np.asarray(state["key_pose"], np.float64), rel)
            u2, d2 = rel[1] * rel[1] + rel[2] * rel[2], key_dist * key_dist
            share = min_share * float(votes)
            margins.take("key_rot", [abs(abs(rel[0]) - key_rot)])
            margins.take("key_dist", [abs(u2 - d2)])
            margins.take("min_share", [abs(float(count) - share)])
            replace = bool(abs(rel[0]) > key_rot or u2 > d2 or float(count) < share)
            age, misses = (0 if replace else int(state["key_age"]) + 1), 0
            if not replace:
                new["key_rel"] = rel.copy()
        else:
            replace = int(state["key_misses"]) + 1 > max_misses
            age = 0 if replace else int(state["key_age"]) + 1
            misses = 0 if replace else int(state["key_misses"]) + 1
    if replace:
        new.update(key_ranges=gated, key_pose=pose.copy(), key_rel=np.zeros(3))
    new.update(key_valid=np.uint8(1), key_age=np.int32(age), key_misses=np.int32(misses), pose=pose.copy())
    c1, s1 = np.cos(pose[2]), np.sin(pose[2])
    good = bool(out["ok"])
    out.update(key_replaced=np.uint8(replace), rot=np.array([c1, -s1, s1, c1]).astype(np.float32), trans=pose[:2].copy(),
               flow_trans=(pose[:2] - old[:2]) if good else np.zeros(2), margins=margins)
    return new, out


OUT_FLOATS, OUT_EXACT = ("motion", "rms", "obs", "flow_residual", "rot", "trans", "flow_trans"), \
    ("count", "ok", "iters_used", "key_replaced", "corr")
STATE_FLOATS, STATE_EXACT = ("key_pose", "key_rel", "pose"), ("key_valid", "key_age", "key_misses", "key_ranges")


def run_sequence(scans, tab, pose0, persons=None, state=None, sum=np.sum, **kw):
    """The steps of one sensor over scans [T,N] from ``new_state(pose0)`` (or `state`) -> [(state after, outputs)]."""
    state = new_state(scans.shape[1], pose0) if state is None else state
    steps = []
    for t in range(len(scans)):
        state, out = keyframe_oracle(scans[t], tab, state, person=None if persons is None else persons[t], sum=sum, **kw)
        steps.append((state, out))
    return steps


def sequence_tolerance(cases):
    """TOL for device-against-oracle over `cases` = [(args, kwargs) of run_sequence], N8's rule: 100 x the largest
    disagreement of the pairwise and the sequential evaluation in any float of any step (outputs and state), at least
    1e-13, never above 1e-10; everything exact must agree, NaNs included, and every decision margin must be >=
    MARGIN_MIN.  -> (tol, the pairwise results)."""
    worst, results, smallest, decisions = 0.0, [], {}, 0
    for args, kw in cases:
        a, b = run_sequence(*args, **kw), run_sequence(*args, sum=seq_sum, **kw)
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


def assert_step_matches(got_out, got_state, want, tol, what=""):
    """Device outputs and state of one sensor after one step (dicts of arrays) against the oracle's (state, outputs):
    everything discrete and the stored keyframe bitwise, the rest within tol, NaN where the oracle has NaN."""
    for got, ref, exact, floats in ((got_out, want[1], OUT_EXACT, OUT_FLOATS), (got_state, want[0], STATE_EXACT, STATE_FLOATS)):
        for key in exact:
            x, y = np.asarray(got[key]), np.asarray(ref[key])
            assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True), (what, key, x, y)
        for key in floats:
            if key not in got:
                continue
            x, y = np.asarray(got[key], np.float64).reshape(-1), np.asarray(ref[key], np.float64).reshape(-1)
            assert np.array_equal(np.isnan(x), np.isnan(y)), (what, key)
            fin = np.isfinite(y)
            err = np.abs(x[fin] - y[fin]).max(initial=0.0)
            assert err <= tol, (what, key, err, tol)


# ---------------------------------------------------------------- scenes
def sequence(T, seed, N=450, noise=0.01, angle_inc=np.radians(0.5), step=None, people=False):
    """T scans of one sensor in a seeded room -> (scans float32 [T,N], poses [T,3], gate or None).  step(t, pose, rng,
    start) -> the next pose (start: the pose at t = 0); default: the steps of ``trajectory`` (tests/test_scan_match.py).  people: every scan gets
    ``add_people`` -> gate = (inst [T,N] int32, num [T] int32, det_cls [T,N], person [T,N] bool)."""
    rng = np.random.default_rng(seed)
    phi = R.laser_phi(angle_inc, N)
    segs = make_room(rng)
    pose = np.concatenate([rng.uniform(-0.5, 0.5, 2), rng.uniform(-np.pi, np.pi, 1)])
    if step is None:
        step = lambda t, p, g, p0: p + np.concatenate([g.uniform(-0.05, 0.05, 2), g.uniform(-0.03, 0.03, 1)])
    scans, poses, start = np.zeros((T, N), np.float32), np.zeros((T, 3)), pose.copy()
    for t in range(T):
        poses[t] = pose
        scans[t] = (ray_cast(segs, pose, phi) + rng.normal(0, 1.0, N) * noise).astype(np.float32)
        pose = step(t, pose, rng, start)
    if not people:
        return scans, poses, None
    got = [add_people(scans[t], rng) for t in range(T)]
    scans = np.stack([g[0] for g in got])
    inst, num, cls = np.stack([g[1] for g in got]), np.array([g[2] for g in got], np.int32), np.stack([g[3] for g in got])
    return scans, poses, (inst, num, cls, np.stack([person_points(inst[t], num[t], cls[t]) for t in range(T)]))


def still(t, pose, rng, start):
    return pose


def sway(t, pose, rng, start):
    """+-0.12 m along x and +-0.15 rad around the pose at t = 0, one period in 20 scans."""
    a = 2 * np.pi * (t + 1) / 20.0
    return start + np.array([0.12 * np.sin(a), 0.0, 0.15 * np.sin(a)])


def walk(t, pose, rng, start):
    """The steps of ``trajectory`` plus 0.04 m per scan forward."""
    pose = pose + np.concatenate([rng.uniform(-0.05, 0.05, 2), rng.uniform(-0.03, 0.03, 1)])
    return pose + np.array([0.04 * np.cos(pose[2]), 0.04 * np.sin(pose[2]), 0.0])


def scenario(name, seed):
    if name == "still":
        return sequence(60, seed, step=still)
    if name == "walk":
        return sequence(40, seed, step=walk)
    return sequence(60, seed, step=sway)


def scan_to_scan(scans, tab, pose0, **kw):
    """Dead reckoning as the streaming detector runs method="scan_match": every pair starts from the previous motion
    (from rest after a failed pair), pof_pose_advance composes an ok motion.  -> poses [T,3]."""
    poses, pose, motion = [np.asarray(pose0, np.float64)], np.asarray(pose0, np.float64), np.zeros(3)
    for t in range(1, len(scans)):
        res = match_oracle(scans[t - 1], scans[t], tab, init=motion, **kw)
        motion = res["motion"]
        if res["ok"]:
            pose = compose(pose, motion)
        poses.append(pose)
    return np.stack(poses)


def position_error(est, true):
    return float(np.hypot(est[:, 0] - true[:, 0], est[:, 1] - true[:, 1]).max())


TAB = angle_table(450)
_DRIFT = {}


def drift(name):
    """-> [(keyframe error, scan-to-scan error, keyframes replaced after the seeding)] over SEEDS, computed once."""
    if name not in _DRIFT:
        rows = []
        for seed in SEEDS:
            scans, poses, _ = scenario(name, seed)
            steps = run_sequence(scans, TAB, poses[0], **SETTINGS)
            key = position_error(np.stack([s["pose"] for s, _ in steps]), poses)
            pair = position_error(scan_to_scan(scans, TAB, poses[0], **DEFAULTS), poses)
            replaced = sum(int(o["key_replaced"]) for _, o in steps[1:])
            assert all(o["ok"] for _, o in steps[1:])
            print("%s seed %d: keyframe %.3e m, scan-to-scan %.3e m, %d keyframes replaced" % (name, seed, key, pair, replaced))
            rows.append((key, pair, replaced))
        _DRIFT[name] = rows
    return _DRIFT[name]


# ---------------------------------------------------------------- tests (no GPU): drift
@pytest.mark.parametrize("name", ["still", "sway"])
def test_the_pose_does_not_drift_in_place(name):
    rows, bound = drift(name), {"still": BOUND_STILL, "sway": BOUND_SWAY}[name]
    for key, pair, replaced in rows:
        assert key < pair and replaced == 0 and key <= bound
    print("%s: worst keyframe %.3e m (bound %.3e), worst scan-to-scan %.3e m"
          % (name, max(r[0] for r in rows), bound, max(r[1] for r in rows)))
    if name == "still":
        assert max(r[0] for r in rows) <= 0.5 * max(r[1] for r in rows)


def test_walking_replaces_keyframes_and_stays_inside_its_bound():
    rows = drift("walk")
    for key, pair, replaced in rows:
        assert key <= BOUND_WALK and replaced >= 1
    print("walk: worst keyframe %.3e m (bound %.3e), worst scan-to-scan %.3e m, %s keyframes replaced"
          % (max(r[0] for r in rows), BOUND_WALK, max(r[1] for r in rows), sorted(r[2] for r in rows)))


# ---------------------------------------------------------------- policy: every branch, the state field by field
def _state_is(state, **want):
    for k, v in want.items():
        assert np.array_equal(np.asarray(state[k]), np.asarray(v), equal_nan=True), (k, state[k], v)


def test_seeding():
    scans, poses, _ = sequence(1, 201)
    scans[0, 5], scans[0, 9] = 25.0, np.inf                    # beyond max_range / not finite: stored as NaN
    start = new_state(450, poses[0])
    state, out = keyframe_oracle(scans[0], TAB, start, **SETTINGS)
    want = scans[0].copy()
    want[[5, 9]] = np.nan
    _state_is(state, key_ranges=want, key_pose=poses[0], key_rel=np.zeros(3), key_valid=1, key_age=0, key_misses=0,
              pose=poses[0])
    assert state["key_ranges"].dtype == np.float32
    assert out["ok"] == 0 and np.isnan(out["motion"]).all() and np.isnan(out["rms"]) and out["count"] == 0
    assert out["iters_used"] == 0 and out["obs"] == 0.0 and out["key_replaced"] == 1
    assert (out["corr"] == -1).all() and np.isnan(out["flow_residual"]).all()
    assert np.array_equal(out["trans"], poses[0][:2]) and np.array_equal(out["flow_trans"], np.zeros(2))
    c, s = np.cos(poses[0][2]), np.sin(poses[0][2])
    assert np.array_equal(out["rot"], np.array([c, -s, s, c]).astype(np.float32))
    _state_is(start, key_valid=0, pose=poses[0])                # the oracle works on a copy


def _until_replaced(scans, poses, **kw):
    steps = run_sequence(scans, TAB, poses[0], **dict(SETTINGS, **kw))
    first = next(t for t in range(1, len(steps)) if steps[t][1]["key_replaced"])
    return steps, first


def test_replacement_by_distance():
    forward = lambda t, p, g, p0: p + np.array([0.11 * np.cos(p[2]), 0.11 * np.sin(p[2]), 0.0])
    scans, poses, _ = sequence(6, 202, step=forward)
    steps, t = _until_replaced(scans, poses)
    assert t == 3                                              # 0.11, 0.22 and then 0.33 m from the keyframe
    for k in range(1, t):
        s, o = steps[k]
        _state_is(s, key_age=k, key_misses=0, key_pose=poses[0], key_rel=o["motion"], key_ranges=steps[0][0]["key_ranges"])
        assert o["ok"] and not o["key_replaced"] and np.hypot(*o["motion"][1:]) <= 0.3
    s, o = steps[t]
    assert o["ok"] and np.hypot(*o["motion"][1:]) > 0.3 and abs(o["motion"][0]) <= 0.3 and o["count"] >= 0.5 * 450
    _state_is(s, key_age=0, key_misses=0, key_rel=np.zeros(3), key_pose=s["pose"], key_ranges=scans[t], key_valid=1)
    assert np.array_equal(s["pose"], compose(poses[0], o["motion"]))
    assert np.array_equal(o["flow_trans"], s["pose"][:2] - steps[t - 1][0]["pose"][:2])
    assert position_error(np.stack([x["pose"] for x, _ in steps]), poses) <= BOUND_WALK
    # the next scan is matched against the new keyframe, from rest
    s2, o2 = steps[t + 1]
    assert o2["ok"] and np.hypot(*o2["motion"][1:]) < 0.15 and s2["key_age"] == 1


def test_replacement_by_rotation_when_turning_in_place():
    scans, poses, _ = sequence(6, 203, step=lambda t, p, g, p0: p + np.array([0.0, 0.0, 0.08]))
    steps, t = _until_replaced(scans, poses)
    s, o = steps[t]
    assert t == 4 and o["ok"] and abs(o["motion"][0]) > 0.3 and np.hypot(*o["motion"][1:]) < 0.05
    assert o["count"] >= 0.5 * 450
    _state_is(s, key_age=0, key_rel=np.zeros(3), key_pose=s["pose"], key_ranges=scans[t])
    assert abs(s["pose"][2] - poses[t][2]) < 1e-3


def test_replacement_by_min_share_after_a_scene_change():
    scans, poses, _ = sequence(3, 204, step=still)
    changed = scans[2].copy()
    changed[:250] = np.maximum(changed[:250] - 2.0, 0.3)       # something large moved in front of 250 beams
    steps = run_sequence(np.stack([scans[0], scans[1], changed]), TAB, poses[0], **SETTINGS)
    (s1, o1), (s2, o2) = steps[1], steps[2]
    assert o1["ok"] and not o1["key_replaced"] and o1["count"] > 400
    assert o2["ok"] and o2["key_replaced"] and 3 <= o2["count"] < 0.5 * 450
    assert abs(o2["motion"][0]) < 0.3 and np.hypot(*o2["motion"][1:]) < 0.3          # only the share test fired
    _state_is(s2, key_age=0, key_misses=0, key_rel=np.zeros(3), key_pose=s2["pose"], key_ranges=changed)
    assert np.array_equal(s2["pose"], compose(poses[0], o2["motion"]))


def test_a_failed_match_leaves_pose_and_key_and_max_misses_re_anchors():
    c0, c1 = corridor()
    pose0 = np.array([1.0, 2.0, 0.5])
    steps = run_sequence(np.stack([c0, c1, c1, c1]), TAB, pose0, **dict(SETTINGS, max_misses=1))
    key0 = steps[0][0]["key_ranges"]
    assert np.isnan(key0).sum() > 0 and np.array_equal(np.isnan(key0), ~(c0 < 20.0))
    s, o = steps[1]                                           # fails: the motion along the corridor is not observable
    assert o["ok"] == 0 and o["count"] > 100 and o["obs"] <= 1e-6 and np.isnan(o["motion"]).all() and np.isnan(o["rms"])
    assert o["key_replaced"] == 0 and (o["corr"] == -1).all() and np.array_equal(o["flow_trans"], np.zeros(2))
    _state_is(s, pose=pose0, key_pose=pose0, key_rel=np.zeros(3), key_ranges=key0, key_age=1, key_misses=1, key_valid=1)
    s, o = steps[2]                                           # the second miss in a row is beyond max_misses = 1
    assert o["ok"] == 0 and o["key_replaced"] == 1 and np.isnan(o["motion"]).all()
    _state_is(s, pose=pose0, key_pose=pose0, key_rel=np.zeros(3), key_age=0, key_misses=0,
              key_ranges=np.where(c1 < 20.0, c1, np.float32(np.nan)))
    s, o = steps[3]
    assert o["ok"] == 0 and o["key_replaced"] == 0 and s["key_misses"] == 1 and s["key_age"] == 1
    # max_misses = 0: the first failure re-anchors
    steps = run_sequence(np.stack([c0, c1]), TAB, pose0, **dict(SETTINGS, max_misses=0))
    assert steps[1][1]["key_replaced"] == 1 and steps[1][0]["key_misses"] == 0


def test_a_key_rel_that_is_not_finite_starts_from_zeros():
    scans, poses, _ = sequence(2, 205)
    seeded = run_sequence(scans[:1], TAB, poses[0], **SETTINGS)[0][0]
    rest, out_rest = keyframe_oracle(scans[1], TAB, seeded, **SETTINGS)
    for bad in ([np.nan, 0.1, 0.1], [0.0, np.inf, 0.0]):
        s, o = keyframe_oracle(scans[1], TAB, dict(seeded, key_rel=np.array(bad)), **SETTINGS)
        assert np.array_equal(o["motion"], out_rest["motion"]) and o["iters_used"] == out_rest["iters_used"]
        _state_is(s, **rest)
    assert out_rest["ok"]


def test_people_in_the_scan_that_becomes_the_keyframe_are_never_vertices():
    scans, poses, gate = sequence(3, 206, people=True)
    person = gate[3]
    steps = run_sequence(scans, TAB, poses[0], persons=person, **SETTINGS)
    key = steps[0][0]["key_ranges"]
    assert np.isnan(key[person[0]]).all() and np.array_equal(key[~person[0]], scans[0][~person[0]])
    assert (gate[0][0][~person[0]] > 0).any()                  # the low-score detection's wall points stay vertices
    for t in (1, 2):
        o = steps[t][1]
        assert o["ok"] and not o["key_replaced"]
        hit = o["corr"][o["corr"] >= 0]
        assert not person[0][hit].any() and (o["corr"][person[t]] == -1).all()
        assert o["count"] <= 450 - person[t].sum()


# ---------------------------------------------------------------- margins: the committed cases of the GPU tests
# N -> B, angle increment (degrees), range noise (m), window, seed, key_dist: the shapes of tests/test_scan_match_gpu.py;
# key_dist is small enough for a replacement inside the T scans
SHAPES = {450: (3, 0.5, 0.01, 16, 301, 0.08), 512: (2, 0.5, 0.01, 16, 311, 0.08), 513: (2, 0.5, 0.01, 16, 321, 0.08),
          4096: (1, 0.05, 0.0, 64, 333, 0.08)}
T_GPU = 6
VARIANTS = ("plain", "huber", "gated")


def shape_case(N, variant):
    """-> (angle increment, scans [T,B,N], poses [T,B,3], gate per sensor or None, settings)."""
    B, inc, noise, window, seed, key_dist = SHAPES[N]
    seqs = [sequence(T_GPU, seed + b, N=N, noise=noise, angle_inc=np.radians(inc), step=walk, people=variant == "gated")
            for b in range(B)]
    kw = dict(SETTINGS, window=window, key_dist=key_dist)
    if variant == "plain":
        kw["huber_delta"] = 0.0
    return (np.radians(inc), np.stack([s[0] for s in seqs], axis=1), np.stack([s[1] for s in seqs], axis=1),
            [s[2] for s in seqs] if variant == "gated" else None, kw)


def shape_oracle(N, variant):
    """The committed case through ``sequence_tolerance`` -> (case, tol, [steps of sensor b])."""
    case = shape_case(N, variant)
    inc, scans, poses, gates, kw = case
    tab = angle_table(N, inc)
    tol, steps = sequence_tolerance([((scans[:, b], tab, poses[0, b]),
                                      dict(kw, persons=None if gates is None else gates[b][3]))
                                     for b in range(scans.shape[1])])
    return case, tol, steps


def rotating_case():
    """Turning 0.1 rad per scan with the keyframe held: up to 57 beams of the scan project outside the keyframe's
    field of view, more than the window."""
    scans, poses, _ = sequence(6, 341, step=lambda t, p, g, p0: p + np.array([0.01, 0.0, 0.1]))
    return scans, poses, dict(SETTINGS, key_rot=1.0, key_dist=1.0)


@pytest.mark.parametrize("N", sorted(SHAPES))
def test_summation_order_the_tolerance_rule_and_the_decision_margins(N):
    for variant in VARIANTS:
        case, tol, steps = shape_oracle(N, variant)
        replaced = [sum(int(o["key_replaced"]) for _, o in s[1:]) for s in steps]
        print("N=%d %s: keyframes replaced per sensor %s" % (N, variant, replaced))
        assert all(r >= 1 for r in replaced) and all(o["ok"] for s in steps for _, o in s[1:])


def test_margins_of_the_rotating_case_and_points_outside_the_field_of_view():
    scans, poses, kw = rotating_case()
    tol, (steps,) = sequence_tolerance([((scans, TAB, poses[0]), kw)])
    last = steps[-1][1]
    assert last["ok"] and not any(o["key_replaced"] for _, o in steps[1:]) and abs(last["motion"][0] - 0.5) < 5e-3
    # rotating to the left: the scan's last beams look past the keyframe's field of view and find nothing
    outside = int(round(0.5 / np.radians(0.5))) - 16
    assert (last["corr"][450 - outside:] == -1).all() and (last["corr"][:200] >= 0).any() and last["corr"].max() == 449
    assert position_error(np.stack([s["pose"] for s, _ in steps]), poses) <= BOUND_WALK


def test_margins_of_the_streaming_cases():
    for name in ("still", "walk"):
        for b in range(2):
            scans, poses, _ = scenario(name, SEEDS[b])
            sequence_tolerance([((scans[:9], TAB, poses[0]), SETTINGS)])


# ---------------------------------------------------------------- host side
def test_abi_and_python_surface():
    import ctypes
    import os
    from planar_optical_flow_amd import _lib, build, ops
    build.build(verbose=False)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pof_abi.h")).read()
    assert "pof_keyframe_match" in _lib.SIGNATURES and "int pof_keyframe_match(" in header
    assert "N9 keyframe scan matching" in header and "tests/test_keyframe.py" in header
    assert len(_lib.SIGNATURES["pof_keyframe_match"][1]) == 41
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "pof_keyframe_match") and hasattr(_lib.load(), "pof_keyframe_match")
    assert ops.KeyframeState._fields == ("key_ranges", "key_pose", "key_rel", "key_valid", "key_age", "key_misses", "pose")
    assert ops.KeyframeMatch._fields == ("motion", "count", "rms", "ok", "iters_used", "obs", "key_replaced", "corr",
                                         "flow_residual")
    assert callable(ops.keyframe_buffers) and callable(ops.keyframe_reset) and callable(ops.keyframe_match_buffers)
    # the library's own argument checks, before any launch: no pointer is dereferenced
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    g = lambda kw, k, d: kw.get(k, d)
    args = lambda **kw: [one, one, None, None, None, 0.5, 20.0, g(kw, "window", 16), g(kw, "gate", 0.5),
                         g(kw, "max_gap", 0.3), g(kw, "huber_delta", 0.05), g(kw, "iters", 16), 1e-7, 1e-7, 1e-6,
                         g(kw, "key_dist", 0.3), g(kw, "key_rot", 0.3), g(kw, "min_share", 0.5), g(kw, "max_misses", 2),
                         g(kw, "B", 1), g(kw, "N", 450)] + [one] * 14 + [None] * 6
    for bad in (dict(window=0), dict(window=65), dict(iters=0), dict(iters=33), dict(gate=-1.0), dict(max_gap=-0.1),
                dict(huber_delta=-0.05), dict(gate=float("nan")), dict(B=-1), dict(N=0), dict(key_dist=-0.1),
                dict(key_rot=-0.1), dict(min_share=-0.5), dict(key_dist=float("nan")), dict(key_rot=float("nan")),
                dict(min_share=float("nan")), dict(max_misses=-1)):
        assert lib.pof_keyframe_match(*args(**bad)) == _lib.POF_E_BADARG, bad
    assert lib.pof_keyframe_match(*args(N=4097)) == _lib.POF_E_SHAPE
    assert lib.pof_keyframe_match(*args(B=0)) == _lib.POF_OK
    for missing in list(range(21, 35)):                        # every state and output pointer is required
        a = args()
        a[missing] = None
        assert lib.pof_keyframe_match(*a) == _lib.POF_E_BADARG, missing
    a = args()
    a[2] = one                                                 # the instance mask without the other NMS results
    assert lib.pof_keyframe_match(*a) == _lib.POF_E_BADARG


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    import torch
    from planar_optical_flow_amd import ops
    B, N = 2, 8
    cur, tab = torch.ones(B, N), torch.zeros(3 * N, dtype=torch.float64)
    state = ops.keyframe_buffers(B, N, "cpu")
    assert [tuple(t.shape) for t in state] == [(B, N), (B, 3), (B, 3), (B,), (B,), (B,), (B, 3)]
    assert [t.dtype for t in state] == [torch.float32, torch.float64, torch.float64, torch.uint8, torch.int32,
                                        torch.int32, torch.float64]
    with pytest.raises(TypeError):
        ops.keyframe_match(cur, tab, state)
    for bad in (dict(window=0), dict(window=65), dict(iters=0), dict(iters=33), dict(gate=-0.5), dict(max_gap=-0.3),
                dict(huber_delta=-1.0), dict(gate=float("nan")), dict(key_dist=-0.3), dict(key_rot=float("nan")),
                dict(min_share=-0.1), dict(max_misses=-1),
                dict(instance_mask=torch.zeros(B, N, dtype=torch.int32), num_det=torch.zeros(B, dtype=torch.int32))):
        with pytest.raises(ValueError):
            ops.keyframe_match(cur, tab, state, **bad)
    sig = inspect.signature(ops.keyframe_match)
    assert list(sig.parameters) == ["ranges_cur", "tab", "state", "instance_mask", "num_det", "det_cls", "cls_thresh",
                                    "max_range", "window", "gate", "max_gap", "huber_delta", "iters", "eps_theta",
                                    "eps_u", "min_pivot", "key_dist", "key_rot", "min_share", "max_misses", "out", "rot",
                                    "trans", "flow_trans"]
    assert {k: sig.parameters[k].default for k in SETTINGS} == SETTINGS
    assert all(p.kind is p.KEYWORD_ONLY for p in list(sig.parameters.values())[3:])
    # keyframe_reset: tensor operations in place
    for t in state:
        t.fill_(3)
    ops.keyframe_reset(state, pose=[1.0, 2.0, 0.5])
    assert all(not t.any() for t in state[:6]) and torch.equal(state.pose, torch.tensor([[1.0, 2.0, 0.5]] * B, dtype=torch.float64))
    ops.keyframe_reset(state)
    assert not state.pose.any()


def test_utils_and_streaming_signatures():
    from planar_optical_flow_amd.src.utils import utils as u
    from planar_optical_flow_amd.streaming import StreamingDetector
    sig = inspect.signature(u.KeyframeOdometry.__init__)
    assert list(sig.parameters) == ["self", "scan_phi", "kw"] and sig.parameters["kw"].kind is inspect.Parameter.VAR_KEYWORD
    assert list(inspect.signature(u.KeyframeOdometry.update).parameters) == ["self", "scan", "pred_cls", "pred_reg"]
    assert list(inspect.signature(u.KeyframeOdometry.reset).parameters) == ["self", "pose"]
    src = inspect.getsource(StreamingDetector)
    for word in ('"keyframe"', "keyframe_match", "_key_state"):
        assert word in src, word
    # the detector's defaults are no literals in its source any more: they are what it hands the stage
    from planar_optical_flow_amd.streaming import stage_settings
    kw = stage_settings("ego_motion", {}, 0.5, "keyframe")
    assert {k: kw[k] for k in ("key_dist", "key_rot", "min_share", "max_misses")} == \
        dict(key_dist=0.3, key_rot=0.3, min_share=0.5, max_misses=2)
