"""Person tracks (pof_track_update, N7) without a GPU: ``track_step`` is the float64 NumPy restatement of the step in
include/pof_abi.h, checked here against the textbook matrix Kalman filter, scenario truths and the lifecycle rules;
tests/test_tracks_gpu.py imports it and the scenarios below and holds the device to them.

The crossing scenario (``walkers``): six people, two of whom pass head-on 0.25 m apart at 0.1 m/scan each; one, who
runs at 0.2 m/scan, drops out for the two scans after the first that sees them, so a track without a velocity of its
own waits 0.6 m behind, outside the gate, while the flow carries a track along; position noise 0.03 m, flow noise
0.05 m/scan; the rows of a scan are permuted, as an NMS rank is, and two rows of every scan are detections below the
score threshold that must take no part."""
import os

import numpy as np
import pytest

SETTINGS = dict(gate=0.5, q=1e-4, r_pos=2.5e-3, r_vel=2.5e-3, v0_var=0.25, max_misses=3, min_hits=3)
PERSISTENT = ("track_id", "track_state", "track_cov", "track_hits", "track_misses", "track_age", "next_id")
OUTPUTS = ("track_det", "track_confirmed", "det_track", "point_track", "dropped")
FLOAT_FIELDS = ("track_state", "track_cov")
INT_FIELDS = tuple(k for k in PERSISTENT + OUTPUTS if k not in FLOAT_FIELDS)
SEEDS = tuple(range(100, 140))                                 # 40 seeds x 30 scans
SCANS = 30
DROPOUT = (2, (1, 2))                                          # walker 2 is not detected in these scans


# ---------------------------------------------------------------- restatement of the step, one sensor
def new_state(M, N):
    """What ops.track_buffers holds for one sensor."""
    i32 = lambda *s: np.zeros(s, np.int32)
    return dict(track_id=i32(M), track_state=np.zeros((M, 4)), track_cov=np.zeros((M, 3)), track_hits=i32(M),
                track_misses=i32(M), track_age=i32(M), next_id=np.ones((), np.int32), track_det=i32(M),
                track_confirmed=np.zeros(M, np.uint8), det_track=i32(N), point_track=i32(N), dropped=i32())


def position_update(p, v, cov, z, r_pos):
    a, b, c = cov
    s = a + r_pos
    k1, k2 = a / s, b / s
    r = z - p
    return p + k1 * r, v + k2 * r, (a - k1 * a, b - k1 * b, c - k2 * b)


def velocity_update(p, v, cov, f, r_vel):
    a, b, c = cov
    s = c + r_vel
    k1, k2 = b / s, c / s
    r = f - v
    return p + k1 * r, v + k2 * r, (a - k1 * b, b - k1 * c, c - k2 * c)


def predict(p, v, cov, q):
    a, b, c = cov
    return p + v, v, ((a + b) + (b + c), b + c, c + q)


def track_step(st, xy, flow, valid, num_det, inst, margins=None, gate=0.5, q=1e-4, r_pos=2.5e-3, r_vel=2.5e-3,
               v0_var=0.25, max_misses=3, min_hits=3):
    """One step on the state ``st`` (``new_state``) in place.  xy, flow [N,2] float64, valid [N], num_det, inst [N].
    ``margins``: a list that receives, per greedy decision, the gap between the best and the second-best open cost, and
    once per step the smallest distance of an open cost from the gate."""
    xy, flow = np.asarray(xy, np.float64), np.asarray(flow, np.float64)
    M, N = len(st["track_id"]), len(valid)
    nd = min(max(int(num_det), 0), N)
    S, P = st["track_state"], st["track_cov"]
    live = np.flatnonzero(st["track_id"] != 0)
    for t in live:                                             # 1. predict
        p, v, cov = predict(S[t, :2], S[t, 2:], tuple(P[t]), q)
        S[t, :2], S[t, 2:], P[t] = p, v, cov
        st["track_age"][t] += 1
    cand = np.array([k for k in range(nd) if valid[k] and np.isfinite(xy[k]).all()], dtype=np.int64)   # 2.
    dx = xy[cand, 0][None, :] - S[live, 0][:, None]            # 3. rows: slots ascending, columns: rows ascending
    dy = xy[cand, 1][None, :] - S[live, 1][:, None]
    cost = dx * dx + dy * dy
    with np.errstate(invalid="ignore"):
        open_ = cost <= gate * gate
    if margins is not None and open_.size:
        finite = cost[np.isfinite(cost)]
        if finite.size:
            margins.append(("gate", float(np.abs(finite - gate * gate).min())))
    matched_slot, matched_cand = {}, set()
    while open_.any():                                         # 4. first minimum in slot-major order: the tie rule
        c = np.where(open_, cost, np.inf)
        i, j = np.unravel_index(np.argmin(c), c.shape)
        if margins is not None:
            two = np.sort(c[open_])[:2]
            if len(two) == 2:
                margins.append(("pair", float(two[1] - two[0])))
        matched_slot[int(live[i])] = int(cand[j])
        matched_cand.add(int(cand[j]))
        open_[i, :] = False
        open_[:, j] = False
    for t, k in matched_slot.items():                          # 5.
        p, v, cov = position_update(S[t, :2], S[t, 2:], tuple(P[t]), xy[k], r_pos)
        if np.isfinite(flow[k]).all():
            p, v, cov = velocity_update(p, v, cov, flow[k], r_vel)
        S[t, :2], S[t, 2:], P[t] = p, v, cov
        st["track_hits"][t] += 1
        st["track_misses"][t] = 0
    for t in live:                                             # 6.
        if int(t) not in matched_slot:
            st["track_misses"][t] += 1
            if st["track_misses"][t] > max_misses:
                for key in ("track_id", "track_state", "track_cov", "track_hits", "track_misses", "track_age"):
                    st[key][t] = 0
    born, dropped = {}, 0
    for k in cand:                                             # 7.
        if int(k) in matched_cand:
            continue
        free = np.flatnonzero(st["track_id"] == 0)
        if not len(free):
            dropped += 1
            continue
        t = int(free[0])
        with_flow = bool(np.isfinite(flow[k]).all())
        st["track_id"][t] = st["next_id"]
        st["next_id"] += 1
        S[t, :2] = xy[k]
        S[t, 2:] = flow[k] if with_flow else 0.0
        P[t] = (r_pos, 0.0, r_vel if with_flow else v0_var)
        st["track_hits"][t], st["track_misses"][t], st["track_age"][t] = 1, 0, 0
        born[t] = int(k)
    st["track_det"][:] = -1                                    # 8.
    st["det_track"][:] = 0
    for t, k in list(matched_slot.items()) + list(born.items()):
        if st["track_id"][t] != 0:
            st["track_det"][t] = k
            st["det_track"][k] = st["track_id"][t]
    st["track_confirmed"][:] = (st["track_id"] != 0) & (st["track_hits"] >= min_hits)
    inst = np.asarray(inst)
    own = (inst >= 1) & (inst <= nd)
    st["point_track"][:] = np.where(own, st["det_track"][np.clip(inst - 1, 0, N - 1)], 0)
    st["dropped"][...] = dropped
    return st


def run_steps(seq, M, N, margins=None, **kw):
    """The states after every step of ``seq`` (dicts of xy, flow, valid, num_det, inst), deep-copied."""
    st, out = new_state(M, N), []
    for s in seq:
        track_step(st, s["xy"], s["flow"], s["valid"], s["num_det"], s["inst"], margins=margins, **kw)
        out.append({k: v.copy() for k, v in st.items()})
    return out


def scan_of(xy, flow=None, valid=None, N=None, num_det=None, inst=None):
    """One scan's inputs from a list of centres (and flows): padded to N rows with zeros."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    n = len(xy)
    N = n if N is None else N
    s = dict(xy=np.zeros((N, 2)), flow=np.zeros((N, 2)), valid=np.zeros(N, np.uint8),
             num_det=np.int32(n if num_det is None else num_det), inst=np.zeros(N, np.int32))
    s["xy"][:n] = xy
    s["flow"][:n] = np.zeros((n, 2)) if flow is None else np.asarray(flow, np.float64).reshape(-1, 2)
    s["valid"][:n] = 1 if valid is None else valid
    if inst is not None:
        s["inst"][:len(inst)] = inst
    return s


# ---------------------------------------------------------------- the crossing scenario
def walkers(seed, N=16, with_flow=True, variant=0):
    """-> (seq, rows [SCANS, 6] = the row of walker w in scan t or -1, velocity [6, 2]).  ``variant`` moves the four
    bystanders, so that the sensors of a batch see different people."""
    rng = np.random.default_rng(seed)
    start = np.array([[-1.5, 0.125], [1.5, -0.125], [-4.0, 3.0], [4.0, 3.0], [-4.0, -3.0], [4.0, -3.0]])
    vel = np.concatenate([[[0.1, 0.0], [-0.1, 0.0]], rng.uniform(-0.04, 0.04, (4, 2))])
    heading = rng.uniform(0.5 * np.pi, np.pi)                  # away from the others
    vel[DROPOUT[0]] = 0.2 * np.cos(heading), 0.2 * np.sin(heading)
    start[2:] += 0.5 * variant
    seq, rows = [], np.full((SCANS, 6), -1)
    for t in range(SCANS):
        seen = [w for w in range(6) if not (w == DROPOUT[0] and t in DROPOUT[1])]
        truth = start + vel * t
        z = truth + rng.normal(0.0, 0.03, (6, 2))
        f = vel + rng.normal(0.0, 0.05, (6, 2))
        # two detections under the score threshold next to walkers 0 and 3: present, not valid
        extra = truth[[0, 3]] + rng.normal(0.0, 0.05, (2, 2))
        order = rng.permutation(len(seen) + 2)
        xy, flow, valid = np.zeros((N, 2)), np.zeros((N, 2)), np.zeros(N, np.uint8)
        inst = np.zeros(N, np.int32)
        for r, src in enumerate(order):
            if src < len(seen):
                w = seen[src]
                xy[r], flow[r], valid[r] = z[w], (f[w] if with_flow else np.nan), 1
                rows[t, w] = r
            else:
                xy[r], flow[r] = extra[src - len(seen)], 0.0
        n = len(order)
        inst[:] = rng.integers(0, n + 3, N)                    # points of every instance, and ids beyond num_det
        valid[n] = 1                                           # a row beyond num_det: not a detection
        seq.append(dict(xy=xy, flow=flow, valid=valid, num_det=np.int32(n), inst=inst))
    return seq, rows, vel


def ids_of(states, rows):
    """[SCANS, 6]: the track id the detection of walker w carries in scan t (0: not seen)."""
    return np.array([[st["det_track"][r] if r >= 0 else 0 for r in row] for st, row in zip(states, rows)])


def changed_ids(ids):
    """How many walkers carry more than one id over the scans they are seen in."""
    return sum(len(set(col[col > 0])) != 1 for col in ids.T)


@pytest.fixture(scope="module")
def crossing():
    """Every seed with and without the flow: states, the walkers' ids, the margins of every decision."""
    res = {}
    for flow_on in (True, False):
        for seed in SEEDS:
            seq, rows, vel = walkers(seed, with_flow=flow_on)
            margins = []
            states = run_steps(seq, 16, 16, margins=margins, **SETTINGS)
            res[flow_on, seed] = dict(seq=seq, rows=rows, vel=vel, states=states, ids=ids_of(states, rows),
                                      margins=margins)
    return res


# ---------------------------------------------------------------- 1. the filter
def test_per_axis_filter_equals_the_matrix_kalman_filter():
    """State (x, y, vx, vy), F = [[I, I], [0, I]], Q = diag(0, 0, q, q), P = [[a I, b I], [b I, c I]]; joint update
    with H = I and R = diag(r_pos, r_pos, r_vel, r_vel), or H = [I 0] without the velocity measurement.  Sequential
    scalar updates equal the joint one for a diagonal R, so the difference is rounding."""
    rng = np.random.default_rng(7)
    q, r_pos, r_vel = SETTINGS["q"], SETTINGS["r_pos"], SETTINGS["r_vel"]
    I2, Z2 = np.eye(2), np.zeros((2, 2))
    F = np.block([[I2, I2], [Z2, I2]])
    Q = np.diag([0.0, 0.0, q, q])
    p, v, cov = np.array([1.5, -2.0]), np.array([0.05, 0.08]), (r_pos, 0.0, 0.25)
    x = np.concatenate([p, v])
    P = np.block([[cov[0] * I2, cov[1] * I2], [cov[1] * I2, cov[2] * I2]])
    worst = 0.0
    for step in range(50):
        p, v, cov = predict(p, v, cov, q)
        x, P = F @ x, F @ P @ F.T + Q
        z, f = x[:2] + rng.normal(0, 0.03, 2), x[2:] + rng.normal(0, 0.05, 2)
        with_velocity = bool(rng.integers(0, 2)) if step >= 2 else bool(step)      # both kinds, from the start
        p, v, cov = position_update(p, v, cov, z, r_pos)
        if with_velocity:
            p, v, cov = velocity_update(p, v, cov, f, r_vel)
            H, Rm, meas = np.eye(4), np.diag([r_pos, r_pos, r_vel, r_vel]), np.concatenate([z, f])
        else:
            H, Rm, meas = np.eye(4)[:2], np.diag([r_pos, r_pos]), z
        K = P @ H.T @ np.linalg.inv(H @ P @ H.T + Rm)
        x, P = x + K @ (meas - H @ x), (np.eye(4) - K @ H) @ P
        want_P = np.block([[cov[0] * I2, cov[1] * I2], [cov[1] * I2, cov[2] * I2]])
        worst = max(worst, np.abs(np.concatenate([p, v]) - x).max(), np.abs(want_P - P).max())
    print("per-axis filter against the 4x4 matrix filter over 50 steps: %.3e" % worst)
    assert worst <= 1e-12


# ---------------------------------------------------------------- 2. the crossing scenario
def test_no_decision_of_the_scenario_rests_on_rounding(crossing):
    gaps = [m for r in crossing.values() for kind, m in r["margins"]]
    print("smallest margin of %d decisions: %.3e" % (len(gaps), min(gaps)))
    assert min(gaps) > 1e-9


def test_with_flow_every_walker_keeps_its_id(crossing):
    changed = sum(changed_ids(crossing[True, s]["ids"]) for s in SEEDS)
    withheld = sum(changed_ids(crossing[False, s]["ids"]) for s in SEEDS)
    print("walkers that changed id: %d of %d with flow, %d without" % (changed, 6 * len(SEEDS), withheld))
    assert withheld >= 1                                       # precondition: the scenario discriminates
    assert changed == 0
    for s in SEEDS:
        r = crossing[True, s]
        w, scans = DROPOUT
        assert r["ids"][scans[0] - 1, w] == r["ids"][scans[-1] + 1, w] > 0             # through the dropout
        assert (r["ids"][list(scans), w] == 0).all()
        assert all(st["dropped"] == 0 for st in r["states"])
        assert r["states"][-1]["next_id"] == 7                 # six people, six ids


def test_track_velocity_is_at_most_half_as_noisy_as_the_raw_flow(crossing):
    err_track, err_raw = [], []
    for s in SEEDS:
        r = crossing[True, s]
        for t in range(11, SCANS):
            st = r["states"][t]
            for w in range(6):
                row = r["rows"][t, w]
                if row < 0:
                    continue
                slot = int(np.flatnonzero(st["track_det"] == row)[0])
                err_track.append(st["track_state"][slot, 2:] - r["vel"][w])
                err_raw.append(r["seq"][t]["flow"][row] - r["vel"][w])
    rms = lambda e: float(np.sqrt((np.array(e) ** 2).sum(axis=1).mean()))
    print("velocity rms error: tracks %.4f, raw flow %.4f m/scan (%.1fx)" % (rms(err_track), rms(err_raw),
                                                                              rms(err_raw) / rms(err_track)))
    assert rms(err_track) <= 0.5 * rms(err_raw)


# ---------------------------------------------------------------- 3. lifecycle
def lifecycle_sequence():
    """One track that is seen once and then missed until it goes, while a second person appears in the step in which
    the first slot is freed.  M = 1: the birth has to reuse that slot in the same step."""
    far = [[5.0, 5.0]]
    seq = [scan_of([[0.0, 0.0]], N=4)] + [scan_of([], N=4) for _ in range(3)] + [scan_of(far, N=4), scan_of(far, N=4)]
    return seq


def test_deletion_reuse_and_ids():
    states = run_steps(lifecycle_sequence(), 1, 4, **SETTINGS)
    assert [int(s["track_id"][0]) for s in states] == [1, 1, 1, 1, 2, 2]
    assert [int(s["track_misses"][0]) for s in states] == [0, 1, 2, 3, 0, 0]     # freed at misses = max_misses + 1
    assert [int(s["track_age"][0]) for s in states] == [0, 1, 2, 3, 0, 1]
    assert [int(s["dropped"]) for s in states] == [0] * 6
    assert np.array_equal(states[4]["track_state"][0], [5.0, 5.0, 0.0, 0.0])
    assert int(states[-1]["next_id"]) == 3
    # one step earlier the slot is still held: the newcomer is dropped, not born
    seq = lifecycle_sequence()
    seq[3] = seq[4]
    states = run_steps(seq, 1, 4, **SETTINGS)
    assert int(states[3]["track_id"][0]) == 1 and int(states[3]["dropped"]) == 1 and int(states[3]["track_misses"][0]) == 3
    assert int(states[4]["track_id"][0]) == 2 and int(states[4]["dropped"]) == 0


def crowd_sequence(n=7, steps=4):
    """n people standing 2 m apart."""
    xy = np.stack([2.0 * np.arange(n), np.zeros(n)], axis=1)
    return [scan_of(xy, N=8, inst=[1, 2, 3, 9, 0, -1, 7, 8]) for _ in range(steps)]


def test_ids_increase_confirmation_and_dropped():
    states = run_steps(crowd_sequence(), 5, 8, **SETTINGS)
    for t, st in enumerate(states):
        assert np.array_equal(st["track_id"], [1, 2, 3, 4, 5])                    # ascending rows, lowest slots
        assert int(st["dropped"]) == 2 and int(st["next_id"]) == 6
        assert np.array_equal(st["track_confirmed"], np.full(5, t + 1 >= SETTINGS["min_hits"]))
        assert np.array_equal(st["track_det"], [0, 1, 2, 3, 4])
        assert np.array_equal(st["det_track"], [1, 2, 3, 4, 5, 0, 0, 0])
        # instance ids 1, 2, 3 are tracked people; 9, 0 and -1 are nobody's; 7 is a dropped detection; 8 > num_det
        assert np.array_equal(st["point_track"], [1, 2, 3, 0, 0, 0, 0, 0])
    # ids are never reused: everyone leaves, others come
    seq = crowd_sequence(3, 1) + [scan_of([], N=8)] * 4 + crowd_sequence(2, 1)
    states = run_steps(seq, 5, 8, **SETTINGS)
    assert np.array_equal(states[4]["track_id"], np.zeros(5)) and np.array_equal(states[5]["track_id"], [4, 5, 0, 0, 0])
    seen = np.concatenate([s["track_id"][s["track_id"] > 0] for s in states])
    assert (np.diff(seen[np.sort(np.unique(seen, return_index=True)[1])]) > 0).all()


def excluded_rows_sequence():
    """Rows that are no candidates -- not valid, a NaN or infinite centre, beyond num_det -- next to a track, and a
    NaN flow on the row that is one."""
    first = scan_of([[0.0, 0.0]], flow=[[0.1, 0.0]], N=6)
    nan = np.nan
    second = scan_of([[0.11, 0.0], [0.1, 0.0], [nan, 0.1], [0.1, np.inf], [0.12, 0.01], [0.1, 0.0]], N=6, num_det=5,
                     flow=[[0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [nan, 0.2], [0.0, 0.0]],
                     valid=[0, 0, 1, 1, 1, 1])
    third = scan_of([[3.0, 3.0]], flow=[[nan, nan]], N=6)
    return [first, second, third]


def test_excluded_rows_and_nan_flow():
    s1, s2, s3 = run_steps(excluded_rows_sequence(), 4, 6, **SETTINGS)
    assert np.array_equal(s2["track_id"], [1, 0, 0, 0]) and int(s2["next_id"]) == 2       # nothing else was born
    assert int(s2["track_det"][0]) == 4 and np.array_equal(s2["det_track"], [0, 0, 0, 0, 1, 0])
    # a position-only update: the velocity moved by k2 * r only, with k2 = b / (a + r_pos)
    p, v, cov = predict(s1["track_state"][0, :2], s1["track_state"][0, 2:], tuple(s1["track_cov"][0]), SETTINGS["q"])
    p, v, cov = position_update(p, v, cov, np.array([0.12, 0.01]), SETTINGS["r_pos"])
    assert np.array_equal(s2["track_state"][0], np.concatenate([p, v])) and np.array_equal(s2["track_cov"][0], cov)
    assert np.array_equal(s1["track_cov"][0], [SETTINGS["r_pos"], 0.0, SETTINGS["r_vel"]])
    # a birth without a flow: velocity 0 with variance v0_var
    assert int(s3["track_id"][1]) == 2 and np.array_equal(s3["track_state"][1], [3.0, 3.0, 0.0, 0.0])
    assert np.array_equal(s3["track_cov"][1], [SETTINGS["r_pos"], 0.0, SETTINGS["v0_var"]])


# ---------------------------------------------------------------- 4. ties, exactly representable
def tie_sequences():
    """-> {name: (M, N, seq)}.  All coordinates are dyadic, so equal costs are equal bits."""
    still = [[0.0, 0.0]]
    return {
        # one track at the origin, two candidates at the same distance: rows 1 and 2 (row 0 is far away)
        "rows": (4, 4, [scan_of(still, N=4), scan_of([[8.0, 8.0], [0.25, 0.0], [-0.25, 0.0]], N=4)]),
        # two tracks at x = -0.25 and 0.25, one candidate in the middle
        "slots": (4, 4, [scan_of([[-0.25, 0.0], [0.25, 0.0]], N=4), scan_of(still, N=4)]),
        # the same in slots 63 / 64 and 1 / 65: one lane's second slot against another lane's first
        "lanes": (66, 128, [scan_of(np.stack([4.0 * np.arange(66), np.zeros(66)], axis=1), N=128),
                             scan_of([[4.0 * 63 + 2.0, 0.0], [4.0 * 1 + 2.0, 0.0], [4.0 * 64 + 2.0, 0.0]], N=128)]),
    }


def test_ties_go_to_the_lower_slot_then_the_lower_row():
    ties = tie_sequences()
    kw = dict(SETTINGS, gate=2.5)
    last = {name: run_steps(seq, M, N, **kw)[-1] for name, (M, N, seq) in ties.items()}
    assert int(last["rows"]["track_det"][0]) == 1 and np.array_equal(last["rows"]["det_track"], [2, 1, 3, 0])
    assert np.array_equal(last["slots"]["track_det"][:2], [0, -1]) and np.array_equal(last["slots"]["track_misses"][:2], [0, 1])
    # candidate 0 lies between slots 63 and 64, candidate 1 between 1 and 2, candidate 2 between 64 and 65
    lanes = last["lanes"]
    assert int(lanes["track_det"][63]) == 0 and int(lanes["track_det"][1]) == 1 and int(lanes["track_det"][64]) == 2
    assert int(lanes["track_det"][2]) == -1 and int(lanes["track_det"][65]) == -1


# ---------------------------------------------------------------- 5. ABI
def test_entry_point_is_declared_bound_and_exported():
    import ctypes
    from planar_optical_flow_amd import _lib, build, ops
    assert "pof_track_update" in _lib.SIGNATURES and len(_lib.SIGNATURES["pof_track_update"][1]) == 28
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pof_abi.h")).read()
    assert "int pof_track_update(" in header
    build.build(verbose=False)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "pof_track_update") and hasattr(_lib.load(), "pof_track_update")
    assert hasattr(ops, "track_update") and hasattr(ops, "track_buffers") and hasattr(ops, "track_reset")
    assert ops.TrackState._fields == PERSISTENT + OUTPUTS
    import torch
    with pytest.raises(TypeError):
        ops.track_update(torch.zeros(1, 4, 2, dtype=torch.float64), torch.zeros(1, 4, 2, dtype=torch.float64),
                         torch.zeros(1, 4, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32),
                         torch.zeros(1, 4, dtype=torch.int32), None)


def test_streaming_detector_takes_a_tracks_argument():
    import inspect
    from planar_optical_flow_amd.streaming import StreamingDetector
    assert "tracks" in inspect.signature(StreamingDetector.__init__).parameters
