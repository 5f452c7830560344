"""Map-checked tracks (pof_track_map, N15) without a GPU: ``track_map_oracle`` is the vectorised NumPy restatement of the
comment in include/pof_abi.h and ``track_map_referee`` a literal per-slot reading of the same comment; they are held to
each other on every scene of this file, and the restatement to literal numbers rule by rule on hand-made scenes (M = 4
slots, N = 8 points, no scan), to what the stage is for on ray-cast rooms with people, and to a planted false positive.
tests/test_track_map_gpu.py imports the restatement and the scenes and holds the device to them bit for bit.

Everything here is integers, except the travel test of step 3, whose numbers in the rule scenes are dyadic.

Measured (this file, the restatements of N11, N7, N12 and N15 chained, ``people_scene(seed, 24, 0.06)`` for seeds 1-8,
256 x 256 cells of 0.1 m, defaults): see ``test_walkers_are_free_standing_and_nobody_is_background`` and
``test_a_planted_false_positive_is_background``, which print, and DESIGN.md 8 N15, which records the figures."""
import inspect
import os
import re

import numpy as np
import pytest

from test_grid_map import grid_map_oracle
from test_person_motion import motion_state, people_scene, person_motion_oracle
from test_tracks import SETTINGS as TRACK_SETTINGS
from test_tracks import new_state as new_track_state, track_step

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = dict(occ_thresh=17, free_pct=50, occ_pct=50, min_points=20, min_scans=3, travel=0.5, cap=4096)
STATE_FIELDS = ("ev_id", "ev_points", "ev_free", "ev_occ", "ev_scans", "ev_start", "ev_moved")
STATE_DTYPES = (np.int32, np.int32, np.int32, np.int32, np.int32, np.float64, np.uint8)
OUT_FIELDS = ("det_occ", "track_class", "det_class", "point_class", "class_count")
OUT_DTYPES = (np.int32, np.uint8, np.uint8, np.uint8, np.int32)
INPUTS = ("inst", "num_det", "point_cell", "point_prior", "det_points", "det_free", "track_id", "track_state", "track_det")
SCANS_MAX = 1 << 30
UNDECIDED, FREE_STANDING, UNSUPPORTED, BACKGROUND = 0, 1, 2, 3


# ---------------------------------------------------------------- restatement of the device arithmetic, one sensor
def new_state(M):
    """What ops.track_map_state holds for one sensor."""
    return {k: np.zeros((M, 2) if k == "ev_start" else M, dt) for k, dt in zip(STATE_FIELDS, STATE_DTYPES)}


def class_of(live, points, free, occ, scans, moved, free_pct, occ_pct, min_points, min_scans):
    """Step 4 for arrays of slots, the products in int64."""
    points, free, occ = (np.asarray(v, np.int64) for v in (points, free, occ))
    decided = live & (np.asarray(scans) >= min_scans) & (points >= min_points)
    background = 100 * occ >= occ_pct * points
    standing = (np.asarray(moved) != 0) | (100 * free >= free_pct * points)
    return np.where(~decided, UNDECIDED, np.where(background, BACKGROUND, np.where(standing, FREE_STANDING, UNSUPPORTED))
                    ).astype(np.uint8)


def track_map_oracle(inst, num_det, point_cell, point_prior, det_points, det_free, track_id, track_state, track_det, state,
                     occ_thresh=17, free_pct=50, occ_pct=50, min_points=20, min_scans=3, travel=0.5, cap=4096):
    """One step of one sensor.  inst, point_cell [N] int32, point_prior [N] int16, det_points, det_free [N] int32,
    track_id, track_det [M] int32, track_state [M,4]; ``state`` (``new_state``) is UPDATED IN PLACE.
    -> dict of the five outputs."""
    inst = np.asarray(inst, np.int64)
    N, M = len(inst), len(track_id)
    nd = min(max(int(num_det), 0), N)
    own = (inst >= 1) & (inst <= nd)
    # 0.
    on_occ = own & (np.asarray(point_cell) >= 0) & (np.asarray(point_prior, np.int64) >= occ_thresh)
    det_occ = np.bincount(inst[on_occ] - 1, minlength=N).astype(np.int32)
    # 1.
    ids = np.asarray(track_id, np.int32)
    xy = np.asarray(track_state, np.float64)[:, :2]
    live = ids != 0
    reused = live & (ids != state["ev_id"])
    for k in STATE_FIELDS:
        state[k][~live | reused] = 0
    state["ev_id"][reused] = ids[reused]
    state["ev_start"][reused] = xy[reused]
    # 2.
    k = np.asarray(track_det, np.int64)
    named = live & (k >= 0) & (k < nd)
    kk = np.where(named, k, 0)
    adds = named & (np.asarray(det_points)[kk] > 0)
    for field, per_row in (("ev_points", det_points), ("ev_free", det_free), ("ev_occ", det_occ)):
        state[field][adds] += np.asarray(per_row, np.int32)[kk][adds]                  # int32, as the device adds
    state["ev_scans"][adds & (state["ev_scans"] < SCANS_MAX)] += 1
    fades = adds & (state["ev_points"] > cap)
    for field in ("ev_points", "ev_free", "ev_occ"):
        state[field][fades] >>= 1
    # 3.
    with np.errstate(invalid="ignore"):
        dx, dy = xy[:, 0] - state["ev_start"][:, 0], xy[:, 1] - state["ev_start"][:, 1]
        d2 = dx * dx + dy * dy                                 # two products and one add, each rounded: no FMA
        state["ev_moved"][live & (d2 >= travel * travel)] = 1  # a NaN compares false
    # 4.
    cls = class_of(live, state["ev_points"], state["ev_free"], state["ev_occ"], state["ev_scans"], state["ev_moved"],
                   free_pct, occ_pct, min_points, min_scans)
    owner = np.full(N, M, np.int64)
    np.minimum.at(owner, k[named], np.flatnonzero(named))      # the lower slot stands
    det_class = np.where(owner < M, cls[np.minimum(owner, M - 1)], 0).astype(np.uint8)
    point_class = np.where(own, det_class[np.clip(inst - 1, 0, N - 1)], 0).astype(np.uint8)
    return dict(det_occ=det_occ, track_class=cls, det_class=det_class, point_class=point_class,
                class_count=np.bincount(cls[live], minlength=4).astype(np.int32))


def track_map_referee(inst, num_det, point_cell, point_prior, det_points, det_free, track_id, track_state, track_det, state,
                      occ_thresh=17, free_pct=50, occ_pct=50, min_points=20, min_scans=3, travel=0.5, cap=4096):
    """The same step read off the header's comment slot by slot, in Python numbers (int32 sums wrapped by hand)."""
    wrap = lambda v: (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31
    N, M = len(inst), len(track_id)
    nd = min(max(int(num_det), 0), N)
    det_occ = [0] * N
    for i in range(N):
        if 1 <= int(inst[i]) <= nd and int(point_cell[i]) >= 0 and int(point_prior[i]) >= occ_thresh:
            det_occ[int(inst[i]) - 1] += 1
    out = dict(det_occ=np.array(det_occ, np.int32), track_class=np.zeros(M, np.uint8), det_class=np.zeros(N, np.uint8),
               point_class=np.zeros(N, np.uint8), class_count=np.zeros(4, np.int32))
    named = {}
    for s in range(M):
        tid = int(track_id[s])
        x, y = float(track_state[s][0]), float(track_state[s][1])
        if tid == 0:
            for f in STATE_FIELDS:
                state[f][s] = 0
            continue
        if tid != int(state["ev_id"][s]):
            for f in STATE_FIELDS:
                state[f][s] = 0
            state["ev_id"][s] = tid
            state["ev_start"][s] = (x, y)
        k = int(track_det[s])
        if 0 <= k < nd:
            named.setdefault(k, s)                             # slots ascend: the lower one stands
            if int(det_points[k]) > 0:
                points = wrap(int(state["ev_points"][s]) + int(det_points[k]))
                free = wrap(int(state["ev_free"][s]) + int(det_free[k]))
                occ = wrap(int(state["ev_occ"][s]) + det_occ[k])
                if int(state["ev_scans"][s]) < SCANS_MAX:
                    state["ev_scans"][s] += 1
                if points > cap:
                    points, free, occ = points >> 1, free >> 1, occ >> 1
                state["ev_points"][s], state["ev_free"][s], state["ev_occ"][s] = points, free, occ
        dx, dy = x - float(state["ev_start"][s][0]), y - float(state["ev_start"][s][1])
        if dx * dx + dy * dy >= travel * travel:
            state["ev_moved"][s] = 1
        points, free, occ = (int(state[f][s]) for f in ("ev_points", "ev_free", "ev_occ"))
        if int(state["ev_scans"][s]) < min_scans or points < min_points:
            cls = UNDECIDED
        elif 100 * occ >= occ_pct * points:
            cls = BACKGROUND
        elif state["ev_moved"][s] or 100 * free >= free_pct * points:
            cls = FREE_STANDING
        else:
            cls = UNSUPPORTED
        out["track_class"][s] = cls
        out["class_count"][cls] += 1
    for k, s in named.items():
        out["det_class"][k] = out["track_class"][s]
    for i in range(N):
        if 1 <= int(inst[i]) <= nd:
            out["point_class"][i] = out["det_class"][int(inst[i]) - 1]
    return out


def same_bits(a, b):
    """Equal bit for bit, a NaN equal to any NaN (ev_start of a track whose position is NaN)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        return bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())
    return bool(np.array_equal(a, b))


def run_steps(scene, step=track_map_oracle):
    """The outputs and the state after every step of a scene (``kw``, ``steps``, optionally ``init``: state fields to
    start from), deep-copied."""
    M = len(scene["steps"][0]["track_id"])
    state = new_state(M)
    for k, v in scene.get("init", {}).items():
        state[k][...] = v
    res = []
    for s in scene["steps"]:
        out = step(*[s[k] for k in INPUTS], state, **scene["kw"])
        res.append(dict(out, **{k: v.copy() for k, v in state.items()}))
    return res


# ---------------------------------------------------------------- rule scenes: hand-made inputs, M = 4, N = 8
RM, RN = 4, 8


def rule_step(ids, det, xy=None, points=(), free=(), inst=(), cell=None, prior=None, num_det=3):
    """One step's inputs: ids, det [M]; xy [M,2] (zeros); points, free per row, inst, prior per beam, padded with zeros
    to N; cell per beam (0: inside)."""
    pad = lambda v, dt: np.concatenate([np.asarray(v, dt).reshape(-1), np.zeros(RN - len(v), dt)])
    state = np.zeros((RM, 4))
    state[:, 2:] = 0.125                                       # a velocity: never read
    if xy is not None:
        state[:, :2] = xy
    return dict(inst=pad(inst, np.int32), num_det=np.int32(num_det), point_cell=pad([] if cell is None else cell, np.int32),
                point_prior=pad([] if prior is None else prior, np.int16), det_points=pad(points, np.int32),
                det_free=pad(free, np.int32), track_id=np.asarray(ids, np.int32), track_state=state,
                track_det=np.asarray(det, np.int32))


def _decided(**kw):
    """Settings under which the state given as ``init`` alone decides: nothing is required of the step."""
    return dict(DEFAULTS, **kw)


def rule_scenes():
    """-> {name: scene}; tests/test_track_map_gpu.py runs every one on the device."""
    small = dict(DEFAULTS, min_points=4, min_scans=2)
    nobody = [-1] * RM
    evidence = lambda ids, points, free, occ, scans, moved=(0, 0, 0, 0): dict(
        ev_id=ids, ev_points=points, ev_free=free, ev_occ=occ, ev_scans=scans, ev_moved=moved)
    return {
        "lifecycle": dict(kw=small, steps=[
            rule_step([1, 2, 0, 3], [0, 1, -1, 2], xy=[(1, 1), (2, 2), (9, 9), (3, 3)], points=[5, 6, 7], free=[1, 6, 2],
                      inst=[1, 1, 2, 3, 3, 3, 0, 0], cell=[0, 0, 0, -1, 5, 5, 0, 0],
                      prior=[17, 16, 17, -32768, 17, 40, 99, 99]),
            # slot 1 reused under id 9; its row is >= num_det; slot 0 unmatched; slot 3's row holds no point
            rule_step([1, 9, 0, 3], [-1, 7, -1, 2], xy=[(1, 1), (5, 5), (0, 0), (3, 3)], points=[5, 6, 0, 0, 0, 0, 0, 8],
                      free=[5, 6, 0, 0, 0, 0, 0, 8]),
            # slot 0 freed
            rule_step([0, 9, 0, 3], [-1, 0, -1, 1], xy=[(4, 4), (5, 5), (0, 0), (3, 3)], points=[4, 3], free=[4, 0]),
        ]),
        "cap": dict(kw=dict(small, cap=RN), init=dict(ev_id=[0, 0, 5, 0], ev_scans=[0, 0, SCANS_MAX, 0]), steps=[
            rule_step([1, 2, 5, 0], [0, 1, 2, -1], points=[5, 6, 1], free=[2, 6, 0], inst=[1, 2, 2, 2], prior=[40] * 4),
            rule_step([1, 2, 5, 0], [0, 1, 2, -1], points=[3, 3, 1], free=[1, 1, 1]),
        ]),
        "free ratio": dict(kw=_decided(), steps=[rule_step([1, 2, 3, 4], nobody)],
                           init=evidence([1, 2, 3, 4], [20, 20, 21, 22], [10, 9, 10, 11], [0] * 4, [3] * 4)),
        "occ ratio": dict(kw=_decided(occ_pct=25), steps=[rule_step([1, 2, 3, 4], nobody)],
                          init=evidence([1, 2, 3, 4], [20, 20, 24, 24], [0, 0, 24, 12], [5, 4, 6, 5], [3] * 4,
                                        moved=[0, 0, 1, 0])),
        "minimums": dict(kw=_decided(), steps=[rule_step([1, 2, 3, 0], nobody)],
                         init=evidence([1, 2, 3, 4], [20, 19, 20, 20], [20] * 4, [0] * 4, [3, 3, 2, 3])),
        "travel": dict(kw=_decided(), init=evidence([1, 2, 3, 4], [20] * 4, [0] * 4, [0] * 4, [3] * 4), steps=[
            rule_step([1, 2, 3, 4], nobody, xy=[(0.5, 0.0), (0.5 - 2.0 ** -20, 0.0), (np.nan, 0.0), (0.4375, -0.25)]),
            rule_step([1, 2, 3, 4], nobody),                   # everybody back where the evidence started
        ]),
        "clamped": dict(kw=dict(DEFAULTS, min_points=1, min_scans=1), steps=[
            rule_step([1, 0, 0, 0], [7, -1, -1, -1], points=[0] * 7 + [6], free=[0] * 7 + [6], inst=[8, 8, 9],
                      prior=[40, 40, 40], num_det=100),
            rule_step([1, 0, 0, 0], [7, -1, -1, -1], points=[0] * 7 + [6], free=[0] * 7 + [6], inst=[8, 8, 9],
                      prior=[40, 40, 40], num_det=-3),
        ]),
        "one row twice": dict(kw=dict(DEFAULTS, min_points=1, min_scans=1, occ_pct=25),
                              init=dict(ev_id=[0, 2, 0, 0], ev_moved=[0, 1, 0, 0]), steps=[
            rule_step([1, 2, 3, 0], [2, 2, 1, -1], points=[9, 4, 8], free=[9, 0, 0], inst=[3, 3, 2, 1, 4, 0, -1, 3],
                      prior=[0, 0, 40, 40, 40, 40, 40, 17]),
        ]),
        "occ thresh zero": dict(kw=dict(DEFAULTS, occ_thresh=0), steps=[
            rule_step([0] * 4, nobody, inst=[1, 1, 1, 1, 2, 2], cell=[0, -1, 3, 3, 0, 0],
                      prior=[0, -32768, -1, -32768, 1, -40], num_det=2),
        ]),
    }


@pytest.fixture(scope="module")
def rules():
    return {name: run_steps(scene) for name, scene in rule_scenes().items()}


def test_reuse_free_and_steps_that_add_nothing(rules):
    a, b, c = rules["lifecycle"]
    # occ_thresh at equality (17 counts, 16 does not); the beam without a cell (-32768) counts nowhere; id 0 is nobody's
    assert a["det_occ"].tolist() == [1, 1, 2, 0, 0, 0, 0, 0]
    assert a["ev_id"].tolist() == [1, 2, 0, 3] and a["ev_points"].tolist() == [5, 6, 0, 7]
    assert a["ev_free"].tolist() == [1, 6, 0, 2] and a["ev_occ"].tolist() == [1, 1, 0, 2]
    assert a["ev_scans"].tolist() == [1, 1, 0, 1] and a["ev_start"].tolist() == [[1, 1], [2, 2], [0, 0], [3, 3]]
    assert a["track_class"].tolist() == [0, 0, 0, 0] and a["class_count"].tolist() == [3, 0, 0, 0]
    # reused under id 9: evidence zeroed, ev_start re-seeded; track_det -1, a row >= num_det and a row without points
    assert b["ev_id"].tolist() == [1, 9, 0, 3] and b["ev_points"].tolist() == [5, 0, 0, 7]
    assert b["ev_free"].tolist() == [1, 0, 0, 2] and b["ev_occ"].tolist() == [1, 0, 0, 2]
    assert b["ev_scans"].tolist() == [1, 0, 0, 1] and b["ev_start"].tolist() == [[1, 1], [5, 5], [0, 0], [3, 3]]
    assert b["det_class"].tolist() == [0] * 8                  # row 7 is >= num_det: nobody's
    # freed: every field zero
    assert all(not c[k][0].any() for k in STATE_FIELDS)
    assert c["ev_points"].tolist() == [0, 4, 0, 10] and c["ev_free"].tolist() == [0, 4, 0, 2]
    assert c["ev_occ"].tolist() == [0, 0, 0, 2] and c["ev_scans"].tolist() == [0, 1, 0, 2]
    assert c["track_class"].tolist() == [0, 0, 0, UNSUPPORTED] and c["class_count"].tolist() == [1, 0, 1, 0]
    assert c["det_class"].tolist() == [0, UNSUPPORTED, 0, 0, 0, 0, 0, 0] and not c["ev_moved"].any()


def test_cap_halves_beyond_it_and_scans_saturate(rules):
    a, b = rules["cap"]
    assert a["ev_points"].tolist() == [5, 6, 1, 0] and a["ev_occ"].tolist() == [1, 3, 0, 0]
    # 8 == cap stays; 9 > cap: 9 >> 1, 7 >> 1, 3 >> 1, once; ev_scans is not halved and stops at 2^30
    assert b["ev_points"].tolist() == [8, 4, 2, 0] and b["ev_free"].tolist() == [3, 3, 1, 0]
    assert b["ev_occ"].tolist() == [1, 1, 0, 0] and b["ev_scans"].tolist() == [2, 2, SCANS_MAX, 0]


def test_every_threshold_at_equality(rules):
    # 100 free == free_pct points: 1000 >= 1000; 900 < 1000; 1000 < 1050; 1100 >= 1100
    assert rules["free ratio"][0]["track_class"].tolist() == [1, 2, 2, 1]
    # occ_pct 25: 500 >= 500; 400 < 500; 600 >= 600 outranks moved and an all-free share; 500 < 600 then 1200 >= 1200
    assert rules["occ ratio"][0]["track_class"].tolist() == [3, 2, 3, 1]
    assert rules["occ ratio"][0]["class_count"].tolist() == [0, 1, 1, 2]
    # points == min_points and scans == min_scans decide; one short of either does not; a free slot is zeroed
    got = rules["minimums"][0]
    assert got["track_class"].tolist() == [1, 0, 0, 0] and got["class_count"].tolist() == [2, 1, 0, 0]
    assert got["ev_id"].tolist() == [1, 2, 3, 0] and got["ev_points"].tolist() == [20, 19, 20, 0]


def test_travel_at_equality_is_sticky_and_a_nan_moves_nothing(rules):
    a, b = rules["travel"]
    # d2 = 0.25 == travel^2; just short of it; NaN; 0.19140625 + 0.0625 = 0.25390625
    assert a["ev_moved"].tolist() == [1, 0, 0, 1] and a["track_class"].tolist() == [1, 2, 2, 1]
    assert b["ev_moved"].tolist() == [1, 0, 0, 1] and b["track_class"].tolist() == [1, 2, 2, 1]
    assert not b["ev_start"].any()                             # the start is where the evidence started, not the NaN


def test_clamped_num_det(rules):
    a, b = rules["clamped"]
    assert a["det_occ"].tolist() == [0] * 7 + [2] and a["ev_points"].tolist() == [6, 0, 0, 0]
    assert a["det_class"].tolist() == [0] * 7 + [1] and a["point_class"].tolist() == [1, 1, 0, 0, 0, 0, 0, 0]
    # num_det < 0 is 0: nothing is added, no row and no point has a class; the class is still the state's
    assert not b["det_occ"].any() and b["ev_points"].tolist() == [6, 0, 0, 0] and b["ev_scans"].tolist() == [1, 0, 0, 0]
    assert b["track_class"].tolist() == [1, 0, 0, 0] and not b["det_class"].any() and not b["point_class"].any()


def test_two_slots_on_one_row_and_points_of_nobody(rules):
    got = rules["one row twice"][0]
    assert got["det_occ"].tolist() == [1, 1, 1, 0, 0, 0, 0, 0]
    assert got["ev_points"].tolist() == [8, 8, 4, 0] and got["ev_occ"].tolist() == [1, 1, 1, 0]
    assert got["track_class"].tolist() == [UNSUPPORTED, FREE_STANDING, BACKGROUND, 0]
    assert got["det_class"].tolist() == [0, BACKGROUND, UNSUPPORTED, 0, 0, 0, 0, 0]       # row 2: slot 0, the lower one
    assert got["point_class"].tolist() == [2, 2, 3, 0, 0, 0, 0, 2] and got["class_count"].tolist() == [0, 1, 1, 1]


def test_occ_thresh_zero(rules):
    assert rules["occ thresh zero"][0]["det_occ"].tolist() == [1, 1, 0, 0, 0, 0, 0, 0]


# ---------------------------------------------------------------- random legal inputs
def random_scene(seed, N, M, T, every_row=False, **kw):
    """T steps of legal inputs for one sensor: slots that are freed and reused, rows matched with at most one slot,
    det_points / det_free consistent with the points, positions on a random walk with a NaN now and then."""
    rng = np.random.default_rng(seed)
    ids, next_id = np.zeros(M, np.int32), 1
    xy = rng.normal(0.0, 1.0, (M, 2))
    steps = []
    for _ in range(T):
        # mostly few rows -- about as many as slots, or one to three -- so that a row has points enough for the sums of
        # the slots matched with them to pass min_points and, in the lowest slots, cap
        u = rng.random()
        nd = N if every_row or u < 0.2 else int(rng.integers(0, min(N, 2 * M) + 1)) if u < 0.6 else int(rng.integers(1, 4))
        inst = rng.integers(-1 if u < 0.6 else 0, nd + 3 if u < 0.6 else nd + 1, N).astype(np.int32)
        if every_row:
            inst[:] = rng.permutation(N) + 1
        cell = np.where(rng.random(N) < 0.2, -1, rng.integers(0, 4096, N)).astype(np.int32)
        prior = np.where(cell < 0, -32768, rng.integers(-40, 71, N)).astype(np.int16)
        own = (inst >= 1) & (inst <= nd) & (cell >= 0)
        points = np.bincount(inst[own] - 1, minlength=N).astype(np.int32)
        free = np.bincount(inst[own & (prior <= -16)] - 1, minlength=N).astype(np.int32)
        for s in range(M):
            if ids[s] and rng.random() < 0.08:
                ids[s] = 0
            if not ids[s] and rng.random() < 0.5:
                ids[s], next_id = next_id, next_id + 1
                xy[s] = rng.normal(0.0, 1.0, 2)
        xy = xy + rng.normal(0.0, 0.1, (M, 2))
        state = np.concatenate([np.where(rng.random((M, 1)) < 0.03, np.nan, xy), rng.normal(0.0, 0.1, (M, 2))], axis=1)
        state[ids == 0] = 0.0
        det = np.full(M, -1, np.int32)
        live = np.flatnonzero(ids)
        rows = rng.permutation(nd)[:len(live)]
        det[live[:len(rows)]] = rows
        det[rng.random(M) < 0.2] = -1
        steps.append(dict(inst=inst, num_det=np.int32(nd), point_cell=cell, point_prior=prior, det_points=points,
                          det_free=free, track_id=ids.copy(), track_state=state, track_det=det))
    return dict(kw=dict(DEFAULTS, **dict(dict(min_points=min(20, N // 4), cap=N, travel=0.25), **kw)), steps=steps)


def test_referee_equals_the_restatement_on_every_scene():
    scenes = dict(rule_scenes(), **{"random %d" % seed: random_scene(seed, 24, 6, 12, every_row=seed == 3)
                                    for seed in (1, 2, 3)})
    decided = 0
    for name, scene in scenes.items():
        for t, (a, b) in enumerate(zip(run_steps(scene), run_steps(scene, track_map_referee))):
            for k, dt in zip(STATE_FIELDS + OUT_FIELDS, STATE_DTYPES + OUT_DTYPES):
                assert a[k].dtype == dt and same_bits(a[k], b[k]), (name, t, k)
            decided += int((a["track_class"] != 0).sum())
    assert decided > 30


# ---------------------------------------------------------------- the chain N11 -> N7 -> N12 -> N15 on rooms
CHAIN_SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)
PLANTED_SEEDS = (3, 7, 6, 2)
CHAIN_M, CHAIN_SIDE, CHAIN_RES, PLANT_SCANS = 16, 256, 0.1, 8


def run_chain(scene, withheld=None):
    """The restatements of person_motion, track_update, grid_map_update and track_map over a scene, defaults throughout.
    ``withheld``: a person whose points are nobody's in the first PLANT_SCANS scans, so that they are burned into the
    map.  -> per scan the track state, the grid outputs and the N15 outputs and state, copied."""
    N = len(scene["scans"][0]["ranges"])
    origin = scene["poses"][0, :2] - 0.5 * CHAIN_RES * CHAIN_SIDE
    grid = np.zeros((CHAIN_SIDE, CHAIN_SIDE), np.int16)
    pm, tracks, ev, res = motion_state(N), new_track_state(CHAIN_M, N), new_state(CHAIN_M), []
    for t, s in enumerate(scene["scans"]):
        inst = s["inst"]
        if withheld is not None and t < PLANT_SCANS:
            inst = np.where(inst == scene["rows"][t, withheld] + 1, 0, inst).astype(np.int32)
        o = person_motion_oracle(s["ranges"], scene["tab"], inst, s["num_det"], s["det_xy"], s["det_cls"], s["rot"],
                                 s["trans"], pm)
        track_step(tracks, o["det_xy_world"], o["det_flow"], o["det_valid"], s["num_det"], inst, **TRACK_SETTINGS)
        g = grid_map_oracle(s["ranges"], scene["tab"], s["rot"], s["trans"], grid, origin, CHAIN_RES, inst, s["num_det"],
                            s["det_cls"])
        c = track_map_oracle(inst, s["num_det"], g["point_cell"], g["point_prior"], g["det_points"], g["det_free"],
                             tracks["track_id"], tracks["track_state"], tracks["track_det"], ev, **DEFAULTS)
        res.append(dict(c, **{k: v.copy() for k, v in ev.items()}, track_det=tracks["track_det"].copy(),
                        track_id=tracks["track_id"].copy()))
    return res


def slot_of(scene, steps, t, p):
    """The slot matched with person p's detection row in scan t, or -1."""
    s = np.flatnonzero(steps[t]["track_det"] == scene["rows"][t, p])
    return int(s[0]) if len(s) else -1


def travel_of(scene):
    return np.linalg.norm(scene["truth"][-1] - scene["truth"][0], axis=1)


@pytest.fixture(scope="module")
def rooms():
    return {seed: people_scene(seed, 24, 0.06) for seed in CHAIN_SEEDS}


@pytest.fixture(scope="module")
def chains(rooms):
    return {seed: run_chain(scene) for seed, scene in rooms.items()}


def _shares(step, s):
    points = max(int(step["ev_points"][s]), 1)
    return step["ev_free"][s] / points, step["ev_occ"][s] / points


def test_walkers_are_free_standing_and_nobody_is_background(rooms, chains):
    """Measured with these restatements, seeds 1-8, at the last scan (travel: first to last true position): 13 people
    travel >= 0.8 m, every one class 1, with a cumulative free share of 0.13-0.87; of the 7 who travel <= 0.3 m none has
    ev_moved, their free share is 0.02-0.40 and all 7 are class 2 (not asserted: 0.40 is too close to free_pct = 50 to
    hold); the largest occ share of any slot in any scan is 0.03."""
    walkers, slow, worst_occ = [], [], 0.0
    for seed, scene in rooms.items():
        steps, travel = chains[seed], travel_of(scene)
        for step in steps:
            assert not (step["track_class"] == BACKGROUND).any()       # persons are gated out of the map
            live = step["ev_points"] > 0
            worst_occ = max([worst_occ] + list(step["ev_occ"][live] / step["ev_points"][live]))
        last = steps[-1]
        for p, d in enumerate(travel):
            s = slot_of(scene, steps, len(steps) - 1, p)
            if d >= 0.8:
                assert s >= 0 and last["track_class"][s] == FREE_STANDING, (seed, p, d)
                walkers.append(_shares(last, s)[0])
            elif d <= 0.3:
                assert s >= 0 and not last["ev_moved"][s], (seed, p, d)
                slow.append((int(last["track_class"][s]), _shares(last, s)[0]))
    print("walkers (>= 0.8 m): %d, all class 1, free share %.2f-%.2f; slow people (<= 0.3 m): %d, classes %s, free share "
          "%.2f-%.2f; largest occ share of any slot in any scan %.2f"
          % (len(walkers), min(walkers), max(walkers), len(slow), sorted(c for c, _ in slow),
             min(f for _, f in slow), max(f for _, f in slow), worst_occ))
    assert len(walkers) >= 10


def test_a_planted_false_positive_is_background(rooms):
    """A person slower than 0.01 m per scan whose points are nobody's for 8 scans and who is detected from scan 8 on.
    Measured, seeds 3, 7, 6, 2 (one such person each): class 3 from scan 10, the third scan it is detected in, to the
    end; 48, 72, 37 and 25 points then (seed 2 is 5 over min_points: the margin is thin by design); over scans 8-23 an occ
    share of 0.84-0.91 and a free share of 0.00-0.15."""
    planted = 0
    for seed in PLANTED_SEEDS:
        scene = rooms[seed]
        speed, travel = np.linalg.norm(scene["vel"], axis=1), travel_of(scene)
        for p in np.flatnonzero(speed < 0.01):
            steps = run_chain(scene, withheld=int(p))
            T = len(steps)
            slots = [slot_of(scene, steps, t, p) for t in range(T)]
            # the detection's centre and score are there all along, so the track is; without points it gathers nothing
            assert all(s >= 0 for s in slots), (seed, p)
            assert all(steps[t]["ev_points"][slots[t]] == 0 for t in range(PLANT_SCANS)), (seed, p)
            classes = [int(steps[t]["track_class"][slots[t]]) for t in range(PLANT_SCANS, T)]
            third = steps[PLANT_SCANS + 2]
            assert third["ev_scans"][slots[PLANT_SCANS + 2]] == 3 and third["ev_points"][slots[PLANT_SCANS + 2]] >= 20
            assert classes[:2] == [UNDECIDED] * 2 and classes[2:] == [BACKGROUND] * (T - PLANT_SCANS - 2), (seed, p, classes)
            free, occ = _shares(steps[-1], slots[-1])
            print("seed %d person %d: %d points at scan %d, occ share %.2f and free share %.2f over scans %d-%d"
                  % (seed, p, third["ev_points"][slots[PLANT_SCANS + 2]], PLANT_SCANS + 2, occ, free, PLANT_SCANS, T - 1))
            for q in np.flatnonzero(travel >= 0.8):            # the walkers of the scene keep their class
                assert steps[-1]["track_class"][slot_of(scene, steps, T - 1, q)] == FREE_STANDING, (seed, p, q)
            planted += 1
    assert planted >= len(PLANTED_SEEDS)


# ---------------------------------------------------------------- surface
RECORDS = {                                                    # in the form of tests/test_stage_records.py
    "track_map_state": ((2, 4), "TrackMapState", (
        ("ev_id", "int32", (2, 4)), ("ev_points", "int32", (2, 4)), ("ev_free", "int32", (2, 4)),
        ("ev_occ", "int32", (2, 4)), ("ev_scans", "int32", (2, 4)), ("ev_start", "float64", (2, 4, 2)),
        ("ev_moved", "uint8", (2, 4)))),
    "track_map_buffers": ((2, 4, 5), "TrackMap", (
        ("det_occ", "int32", (2, 5)), ("track_class", "uint8", (2, 4)), ("det_class", "uint8", (2, 5)),
        ("point_class", "uint8", (2, 5)), ("class_count", "int32", (2, 4)))),
}


def test_records_and_settings_match_literal_tables():
    import torch
    from planar_optical_flow_amd import ops, streaming
    for fn, (args, cls, fields) in RECORDS.items():
        rec = getattr(ops, fn)(*args, device="cpu")
        assert type(rec) is getattr(ops, cls) and type(rec).__name__ == cls, fn
        assert rec._fields == tuple(f for f, _, _ in fields), fn
        for (f, dtype, shape), t in zip(fields, rec):
            assert (t.dtype, tuple(t.shape), t.device.type) == (getattr(torch, dtype), shape, "cpu") and not t.any(), (fn, f)
    assert ops.TrackMapState.persistent == STATE_FIELDS and ops.TrackMap.persistent == ()
    assert ops.TrackMapState._fields == STATE_FIELDS and ops.TrackMap._fields == OUT_FIELDS
    got = ops.stage_settings(ops.track_map)
    assert got == DEFAULTS and list(got) == list(DEFAULTS)
    assert {k: type(v) for k, v in got.items()} == {k: type(v) for k, v in DEFAULTS.items()}
    assert streaming.stage_defaults("track_map") == DEFAULTS
    assert streaming.stage_settings("track_map", dict(cap=512)) == dict(DEFAULTS, cap=512)
    with pytest.raises(ValueError, match="unknown track_map settings"):
        streaming.stage_settings("track_map", dict(caps=512))
    state = ops.track_map_state(2, 4, device="cpu")
    for t in state:
        t.fill_(3)
    assert ops.track_map_reset(state) is not None and not any(t.any() for t in state)


def test_header_binding_and_wrappers():
    import torch
    from planar_optical_flow_amd import _lib, ops
    from planar_optical_flow_amd.src.utils import utils
    from planar_optical_flow_amd.streaming import StreamingDetector
    text = open(os.path.join(REPO, "include", "pof_abi.h")).read()
    m = re.search(r"\bint\s+pof_track_map\s*\(([^)]*)\)\s*;", text)
    assert m, "include/pof_abi.h does not declare pof_track_map"
    params = [p.strip() for p in m.group(1).split(",")]
    restype, argtypes = _lib.SIGNATURES["pof_track_map"]
    assert restype is _lib._i and len(argtypes) == len(params) == 32
    for p, t in zip(params, argtypes):
        want = _lib._p if "*" in p or p.startswith("pof_stream_t") else _lib._d if p.startswith("double") else _lib._i
        assert t is want, p
    assert "N15" in text and "ev_moved" in text and _lib.load().pof_abi_version() == 1
    for name in ("track_map", "track_map_state", "track_map_buffers", "track_map_reset"):
        assert callable(getattr(ops, name))
    p = inspect.signature(ops.track_map).parameters
    assert list(p)[:5] == ["tracks", "grid_out", "instance_mask", "num_det", "state"] and p["out"].default is None
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(DEFAULTS) + ["out"])
    assert list(inspect.signature(utils.TrackMap.__init__).parameters)[1:] == ["max_tracks", "settings"]
    assert list(inspect.signature(utils.TrackMap.update).parameters)[1:] == ["tracker", "grid"]
    assert callable(utils.TrackMap.reset)
    assert inspect.signature(StreamingDetector.__init__).parameters["track_map"].default is None
    assert callable(StreamingDetector.track_map)
    with pytest.raises(ValueError, match="unknown track_map settings"):
        utils.TrackMap(caps=3)
    # no CPU path
    with pytest.raises(TypeError):
        ops.track_map(ops.track_buffers(1, 4, 8, device="cpu"), ops.grid_map_buffers(1, 8, device="cpu"),
                      torch.zeros(1, 8, dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                      ops.track_map_state(1, 4, device="cpu"))


def test_entry_point_refuses_null_and_bad_arguments():
    import ctypes
    from planar_optical_flow_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "pof_track_map")
    _, argtypes = _lib.SIGNATURES["pof_track_map"]
    assert lib.pof_track_map(*[None if t is _lib._p else 0 for t in argtypes]) == _lib.POF_E_BADARG
    assert lib.pof_track_map(*[None if t is _lib._p else 1 for t in argtypes]) == _lib.POF_E_BADARG
    # with pointers (never followed: every call below is refused, or B is 0): the order of the refusals
    word = (ctypes.c_double * 4)()
    good = dict(B=0, N=8, M=4, occ_thresh=17, free_pct=50, occ_pct=50, min_points=20, min_scans=3, travel=0.5, cap=8)

    def call(**kw):
        v = dict(good, **kw)
        ptrs = [ctypes.cast(word, ctypes.c_void_p)] * 21
        return lib.pof_track_map(*ptrs[:9], v["B"], v["N"], v["M"], *ptrs[9:], v["occ_thresh"], v["free_pct"],
                                 v["occ_pct"], v["min_points"], v["min_scans"], v["travel"], v["cap"], None)

    assert call() == _lib.POF_OK                               # B = 0 with valid pointers
    for bad in (dict(B=-1), dict(N=0), dict(M=0), dict(occ_thresh=-1), dict(free_pct=101), dict(free_pct=-1),
                dict(occ_pct=101), dict(occ_pct=-1), dict(min_points=-1), dict(min_scans=-1), dict(cap=7),
                dict(cap=(1 << 20) + 1), dict(travel=-1.0), dict(travel=float("nan")),
                dict(N=4097, cap=4096), dict(M=257, cap=7)):    # BADARG is checked first
        assert call(**bad) == _lib.POF_E_BADARG, bad
    for bad in (dict(N=4097, cap=4097), dict(M=257), dict(N=4097, M=257, cap=1 << 20)):
        assert call(**bad) == _lib.POF_E_SHAPE, bad
    assert call(N=4096, M=256, cap=1 << 20, free_pct=100, occ_pct=0, travel=0.0, occ_thresh=0) == _lib.POF_OK
