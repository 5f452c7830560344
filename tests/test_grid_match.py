"""Scan-to-grid matching (pof_grid_match, N13) without a GPU: ``grid_match_oracle`` is the NumPy restatement of the
comment in include/pof_abi.h -- float64 for the cells, integers for everything behind them -- checked here rule by rule
on scenes whose numbers are exact (N12's ``axis_beams`` layout, hand-painted grids, and a literal triple loop of the
score rule), and on ray-cast rooms for what the stage is good for: it is silent while the pose is good, it brings a
pose back that lost two scan pairs, and the map stays healthy behind it.  tests/test_grid_match_gpu.py imports the
restatement and the cases and holds the device to them bit for bit.

The search has no transcendental and no float sum: the cell of a point is N12's point_cell arithmetic behind one
rotation by a table row, every operation of it correctly rounded in NumPy and on the device alike, so there is no
ambiguous scene and no tolerance anywhere but the float32 rotation terms a moved pose is written with (one ulp, as
for pof_pose_advance).

Measured with this restatement (``drive``, seeds 11-14: one room each, 225 degree view, N = 450, 1 cm noise, 256 x 256
cells of 0.1 m, 16 scans of about 0.11 m each, scan 13 all NaN so that two pairs fail and 0.22 m are lost): see the
docstrings of the three quality tests, which print their figures, and DESIGN.md 8 N13, which records them.  The
spoiled scan stands two scans in front of the last one because that is where the map-health count can tell the two
runs apart: a wall that lands on cells seen free (lo = -40) lifts them above -free_thresh = -16 with its second hit
(-40 + 17 + 17 = -6), so from the third scan at a shifted pose on the shifted wall hides itself from that count."""
import inspect
import os
import re

import numpy as np
import pytest

from test_grid_map import (BASE_RANGES, CENTRE, CX, CY, DEFAULTS as MAP_DEFAULTS, INF, NAN, RES, RULE_H, RULE_ORIGIN,
                           RULE_W, SPOILED_RANGES, axis_beams, grid_map_oracle, room_scene)
from test_person_motion import IDENTITY
from test_scan_match import angle_table, make_room, match_oracle, ray_cast

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = dict(cls_thresh=0.5, max_range=20.0, reach=4, rotations=9, rot_step=0.01, min_points=50, min_score=20,
                min_gain=8)
OUT_FIELDS = ("scores", "best", "score", "votes", "ok", "moved", "correction")
OUT_DTYPES = (np.int32, np.int32, np.int32, np.int32, np.uint8, np.uint8, np.float64)


# ---------------------------------------------------------------- restatement of the device arithmetic, one sensor
def rotation_table(rot_step, rotations):
    """[K,3] = (theta, cos, sin), theta_k = (k - (K - 1) / 2) rot_step; the middle row is exactly (0, 1, 0)."""
    theta = (np.arange(rotations, dtype=np.float64) - (rotations - 1) // 2) * float(rot_step)
    return np.stack([theta, np.cos(theta), np.sin(theta)], axis=1)


def pose_terms(pose):
    """(rot float32 [4], trans [2]) of (x, y, phi), as pof_write_pose_terms forms them."""
    c, s = np.cos(pose[2]), np.sin(pose[2])
    return np.array([c, -s, s, c]).astype(np.float32), np.array([pose[0], pose[1]], np.float64)


def voting_points(ranges, inst=None, num_det=None, det_cls=None, cls_thresh=0.5, max_range=20.0):
    """bool [N]: finite, 0 < r < max_range and no person's point (N12's gate)."""
    r = np.asarray(ranges, np.float32).astype(np.float64)
    N = len(r)
    with np.errstate(invalid="ignore"):
        votes = np.isfinite(r) & (r > 0.0) & (r < max_range)
    if inst is not None:
        nd = min(max(int(num_det), 0), N)
        ids = np.asarray(inst, np.int64)
        row_of = (ids >= 1) & (ids <= nd)
        votes &= ~(row_of & (np.asarray(det_cls, np.float64)[np.where(row_of, ids - 1, 0)] >= cls_thresh))
    return votes


def rotated_cells(ranges, tab, rot, trans, origin, res, c, s):
    """(g_x, g_y) float64 [N] of every point under the table row (c, s): the header's expressions, no FMA."""
    r = np.asarray(ranges, np.float32).astype(np.float64)
    N = len(r)
    tab = np.asarray(tab, np.float64)
    Rm = np.asarray(rot, np.float32).reshape(2, 2).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        px, py = r * tab[N::2], r * tab[N + 1::2]
        qx, qy = c * px - s * py, s * px + c * py
        wx, wy = (Rm[0, 0] * qx + Rm[0, 1] * qy) + float(trans[0]), (Rm[1, 0] * qx + Rm[1, 1] * qy) + float(trans[1])
        return np.floor((wx - float(origin[0])) / res), np.floor((wy - float(origin[1])) / res)


def grid_match_oracle(ranges, tab, rot, trans, pose, grid, origin, res, inst=None, num_det=None, det_cls=None,
                      table=None, cls_thresh=0.5, max_range=20.0, reach=4, rotations=9, rot_step=0.01, min_points=50,
                      min_score=20, min_gain=8):
    """One scan of one sensor against its grid [H,W] int16 (read only).  ranges [N] float32, tab [3N], rot float32 [2,2]
    (or [4]), trans [2], pose [3]; inst [N], num_det, det_cls [N] padded like the NMS outputs, all three or none.
    -> dict of the seven outputs, the new pose, rot [4] float32 and trans (the incoming objects' values without
    ``moved``), and cells [K,N,2] int64 = (g_x, g_y) of every voting point with a finite cell, else (-2^40, -2^40)."""
    R, K = int(reach), int(rotations)
    T, (H, W) = 2 * R + 1, grid.shape
    table = rotation_table(rot_step, K) if table is None else np.asarray(table, np.float64)
    votes = voting_points(ranges, inst, num_det, det_cls, cls_thresh, max_range)
    V = int(votes.sum())
    padded = np.zeros((H + 4 * R, W + 4 * R), np.int64)        # a shifted cell outside the grid adds 0
    padded[2 * R:2 * R + H, 2 * R:2 * R + W] = grid
    scores = np.zeros((K, T, T), np.int64)
    cells = np.full((K, len(votes), 2), -2 ** 40, np.int64)
    for k in range(K):
        gx, gy = rotated_cells(ranges, tab, rot, trans, origin, res, table[k, 1], table[k, 2])
        finite = votes & np.isfinite(gx) & np.isfinite(gy)
        # integers from here on; a cell further than R from the grid reaches none of its cells under any shift
        near = finite & (gx >= -R) & (gx < W + R) & (gy >= -R) & (gy < H + R)
        ix, iy = gx[near].astype(np.int64), gy[near].astype(np.int64)
        cells[k, finite] = np.stack([np.clip(gx[finite], -2.0 ** 40, 2.0 ** 40), np.clip(gy[finite], -2.0 ** 40, 2.0 ** 40)],
                                    axis=1).astype(np.int64)
        for a in range(T):
            for e in range(T):
                scores[k, a, e] = padded[iy + R + a, ix + R + e].sum()
    mid = (K - 1) // 2
    kk, aa, ee = np.meshgrid(np.arange(K), np.arange(T), np.arange(T), indexing="ij")
    d2, kap = (aa - R) ** 2 + (ee - R) ** 2, np.abs(kk - mid)
    flat = np.lexsort((np.arange(K * T * T), kap.ravel(), d2.ravel(), -scores.ravel()))[0]
    k, a, e = np.unravel_index(flat, scores.shape)
    best, zero = int(scores[k, a, e]), int(scores[mid, R, R])                  # Python integers: no overflow
    ok = V >= int(min_points) and best >= int(min_score) * V
    moved = bool(ok and (k, a, e) != (mid, R, R) and best - zero >= int(min_gain) * V)
    dx, dy = int(e) - R, int(a) - R
    pose = np.asarray(pose, np.float64).copy()
    rot4, trans2 = np.asarray(rot, np.float32).reshape(4).copy(), np.asarray(trans, np.float64).copy()
    correction = np.zeros(3)
    if moved:
        correction = np.array([float(dx) * res, float(dy) * res, table[k, 0]])
        pose = pose + correction
        rot4, trans2 = pose_terms(pose)
    return dict(scores=scores.astype(np.int32), best=np.array([k - mid, dy, dx], np.int32),
                score=np.array([best, zero], np.int32), votes=np.int32(V), ok=np.uint8(ok), moved=np.uint8(moved),
                correction=correction, pose=pose, rot=rot4, trans=trans2, cells=cells)


def literal_scores(ranges, tab, rot, trans, grid, origin, res, votes, table, reach):
    """The score rule as the header words it, one Python loop per index: for the small rule scenes only."""
    R, K, (H, W) = reach, len(table), grid.shape
    T = 2 * R + 1
    out = np.zeros((K, T, T), np.int64)
    for k in range(K):
        gx, gy = rotated_cells(ranges, tab, rot, trans, origin, res, table[k, 1], table[k, 2])
        for i in np.flatnonzero(votes):
            if not (np.isfinite(gx[i]) and np.isfinite(gy[i])):
                continue
            x0, y0 = int(gx[i]), int(gy[i])
            for a in range(T):
                for e in range(T):
                    x, y = x0 + (e - R), y0 + (a - R)
                    if 0 <= x < W and 0 <= y < H:
                        out[k, a, e] += int(grid[y, x])
    return out


def run_case(case):
    """The restatement over every sensor of a case -> list of its dicts."""
    return [grid_match_oracle(s["ranges"], case["tab"], s["rot"], s["trans"], s["pose"], s["grid"], s["origin"],
                              case["res"], s.get("inst"), s.get("num_det"), s.get("det_cls"), **case["kw"])
            for s in case["sensors"]]


# ---------------------------------------------------------------- rule scenes: exact numbers
RULE_POSE = np.array([CENTRE[0], CENTRE[1], 0.0])
GATED = dict(inst=(0, 5, 0, 0, 1, -1, 2, 0, 0), num_det=2, det_cls=(0.9, 0.2))
# the cells of BASE_RANGES' four voting beams 1, 4, 5, 6 at the rule pose (tests/test_grid_map.py derives 1, 4 and 6)
BASE_CELLS = {1: (61, 29), 4: (72, CY), 5: (78, 46), 6: (CX, 40)}


def _sensor(ranges, grid, rot=IDENTITY, pose=RULE_POSE, origin=RULE_ORIGIN, inst=None, num_det=None, det_cls=None):
    s = dict(ranges=np.asarray(ranges, np.float32), rot=np.asarray(rot, np.float32).reshape(2, 2).copy(),
             trans=np.asarray(pose[:2], np.float64).copy(), pose=np.asarray(pose, np.float64).copy(),
             grid=np.asarray(grid, np.int16), origin=np.asarray(origin, np.float64))
    if inst is not None:
        cls = np.zeros(len(s["ranges"]))
        cls[:len(det_cls)] = det_cls
        s.update(inst=np.asarray(inst, np.int32), num_det=np.int32(num_det), det_cls=cls)
    return s


def painted(shifts, value=30, cells=BASE_CELLS.values()):
    """A grid with ``value`` on every given cell moved by each (dy, dx) of ``shifts``."""
    g = np.zeros((RULE_H, RULE_W), np.int16)
    for dy, dx in shifts:
        for x, y in cells:
            g[y + dy, x + dx] += value
    return g


def noise_grid(seed):
    return np.random.default_rng(seed).integers(-40, 71, (RULE_H, RULE_W)).astype(np.int16)


def _case(kw, *sensors):
    return dict(tab=axis_beams(), H=RULE_H, W=RULE_W, res=RES, kw=dict(DEFAULTS, **kw), sensors=list(sensors))


def rule_cases():
    """-> {name: case}; a case is dict(tab, H, W, res, kw, sensors=[dict(ranges, rot, trans, pose, grid, origin and the
    NMS results)]).  The tests below say what each is for."""
    few = dict(max_range=3.0, min_points=1, min_score=1, min_gain=1)
    return {
        "noise": _case(few, _sensor(BASE_RANGES, noise_grid(1))),
        "smallest search": _case(dict(few, reach=0, rotations=1), _sensor(BASE_RANGES, noise_grid(2), **GATED)),
        "one off": _case(few, _sensor(BASE_RANGES, painted([(0, 1)]))),
        "two off": _case(few, _sensor(BASE_RANGES, painted([(-2, 1)]))),
        "tie by distance": _case(few, _sensor(BASE_RANGES, painted([(0, 1), (0, -2)]))),
        "tie by rotation": _case(dict(few, rotations=3, rot_step=0.0), _sensor(BASE_RANGES, painted([(0, 1)]))),
        "tie by index": _case(few, _sensor(BASE_RANGES, painted([(0, 1), (0, -1), (1, 0)]))),
        "leaves the grid": _case(dict(DEFAULTS, reach=16, rotations=3, min_points=1, min_score=1, min_gain=1),
                                 _sensor((INF, INF, INF, INF, 0.9375, INF, 5.0, INF, INF), noise_grid(3))),
        "spoiled": _case(dict(few, max_range=2.0), _sensor(SPOILED_RANGES + (), noise_grid(4)),
                         _sensor((INF, NAN, 0.0, -1.0, 2.0, 2.5, 1.0, 1.5, INF), noise_grid(4))),
        "gate": _case(few, _sensor(BASE_RANGES, noise_grid(5), **GATED)),
        "clamped": _case(few, _sensor(BASE_RANGES, noise_grid(6), inst=(0, 0, 0, 0, 9, 0, 10, 0, 0), num_det=100,
                                      det_cls=(0, 0, 0, 0, 0, 0, 0, 0, 0.9)),
                         _sensor(BASE_RANGES, noise_grid(6), inst=(0, 0, 0, 0, 1, 0, 1, 0, 0), num_det=-3, det_cls=(0.9,))),
        "quarter turn": _case(few, _sensor(BASE_RANGES, noise_grid(7), rot=[[0.0, -1.0], [1.0, 0.0]],
                                           pose=(CENTRE[0], CENTRE[1], np.pi / 2))),
        # the gates at equality and one short of it: V = 4, best = 120, zero = 0
        "ok at equality": _case(dict(few, min_points=4, min_score=30, min_gain=30), _sensor(BASE_RANGES, painted([(0, 1)]))),
        "too few points": _case(dict(few, min_points=5, min_score=30, min_gain=30), _sensor(BASE_RANGES, painted([(0, 1)]))),
        "score too low": _case(dict(few, min_points=4, min_score=31, min_gain=30), _sensor(BASE_RANGES, painted([(0, 1)]))),
        "gain too low": _case(dict(few, min_points=4, min_score=30, min_gain=31), _sensor(BASE_RANGES, painted([(0, 1)]))),
        "empty grid": _case(dict(few, min_points=0, min_score=0, min_gain=0),
                            _sensor(BASE_RANGES, np.zeros((RULE_H, RULE_W), np.int16))),
    }


@pytest.fixture(scope="module")
def rules():
    cases = rule_cases()
    return {k: run_case(c) for k, c in cases.items()}


def test_the_middle_row_is_the_grid_maps_point_cell(rules):
    case = rule_cases()["noise"]
    s, o = case["sensors"][0], rules["noise"][0]
    m = grid_map_oracle(s["ranges"], case["tab"], s["rot"], s["trans"], s["grid"].copy(), s["origin"], RES,
                        **dict(MAP_DEFAULTS, max_range=3.0))
    mid = o["cells"][4]
    seen = m["point_cell"] >= 0
    assert seen.sum() == 4 and np.array_equal(mid[seen, 1] * RULE_W + mid[seen, 0], m["point_cell"][seen])
    assert {i: tuple(mid[i]) for i in np.flatnonzero(seen)} == BASE_CELLS
    assert (mid[~seen] == -2 ** 40).all() and o["votes"] == 4
    assert rotation_table(0.01, 9)[4].tolist() == [0.0, 1.0, 0.0]             # the middle row is exact


def test_the_smallest_search_sums_the_priors_of_the_marked_points(rules):
    case = rule_cases()["smallest search"]
    s, o = case["sensors"][0], rules["smallest search"][0]
    m = grid_map_oracle(s["ranges"], case["tab"], s["rot"], s["trans"], s["grid"].copy(), s["origin"], RES, s["inst"],
                        s["num_det"], s["det_cls"], **dict(MAP_DEFAULTS, max_range=3.0))
    marked = m["point_mark"] == 1
    assert marked.sum() == 3 and o["scores"].shape == (1, 1, 1)
    assert o["score"].tolist() == [int(m["point_prior"][marked].astype(np.int64).sum())] * 2
    assert o["best"].tolist() == [0, 0, 0] and o["moved"] == 0                # the only candidate is the zero candidate


def test_every_rule_scene_equals_the_literal_loops(rules):
    for name, case in rule_cases().items():
        kw = case["kw"]
        table = rotation_table(kw["rot_step"], kw["rotations"])
        for s, o in zip(case["sensors"], rules[name]):
            votes = voting_points(s["ranges"], s.get("inst"), s.get("num_det"), s.get("det_cls"), kw["cls_thresh"],
                                  kw["max_range"])
            want = literal_scores(s["ranges"], case["tab"], s["rot"], s["trans"], s["grid"], s["origin"], RES, votes,
                                  table, kw["reach"])
            assert np.array_equal(o["scores"], want) and o["scores"].dtype == np.int32, name
            assert o["votes"] == votes.sum(), name


def test_a_wall_painted_one_and_two_cells_off_is_found(rules):
    one, two = rules["one off"][0], rules["two off"][0]
    assert one["best"].tolist() == [0, 0, 1] and one["score"].tolist() == [120, 0] and one["ok"] and one["moved"]
    assert one["correction"].tolist() == [0.125, 0.0, 0.0] and one["pose"].tolist() == [0.1875, 0.0625, 0.0]
    assert one["trans"].tolist() == [0.1875, 0.0625] and one["rot"].tolist() == [1.0, 0.0, 0.0, 1.0]
    assert two["best"].tolist() == [0, -2, 1] and two["score"].tolist() == [120, 0] and two["moved"]
    assert two["correction"].tolist() == [0.125, -0.25, 0.0] and two["pose"].tolist() == [0.1875, -0.1875, 0.0]
    assert (one["scores"] == 120).sum() == 1 and (two["scores"] == 120).sum() == 1


def test_every_level_of_the_tie_rule(rules):
    d = rules["tie by distance"][0]
    # dx = +1 and dx = -2 both score 120: the shorter translation wins although its flat index is the larger one
    assert (d["scores"] == 120).sum() == 2 and d["scores"][4, 4, 2] == 120 and d["best"].tolist() == [0, 0, 1]
    r = rules["tie by rotation"][0]
    # rot_step = 0: the three rows are the same rotation and score alike; kappa = 0 wins over the lower index of kappa = -1
    assert (r["scores"][:, 4, 5] == 120).all() and r["best"].tolist() == [0, 0, 1] and r["correction"][2] == 0.0
    i = rules["tie by index"][0]
    # (dy, dx) = (0, 1), (0, -1), (1, 0) at the same distance and rotation: the lowest flat index is (0, -1)
    assert (i["scores"] == 120).sum() == 3 and i["best"].tolist() == [0, 0, -1] and i["pose"][0] == 0.0625 - 0.125


def test_a_shifted_cell_outside_the_grid_adds_nothing(rules):
    case = rule_cases()["leaves the grid"]
    s, o = case["sensors"][0], rules["leaves the grid"][0]
    g = s["grid"].astype(np.int64)
    mid = o["cells"][1]
    assert tuple(mid[4]) == (72, CY) and tuple(mid[6]) == (CX, 72) and o["votes"] == 2     # beam 6 ends 8 rows above the grid
    sc = o["scores"][1]
    assert sc[16, 16] == g[CY, 72]                             # no shift: beam 6 adds nothing
    assert sc[16 - 9, 16] == g[CY - 9, 72] + g[63, CX]         # dy = -9 brings it onto the last row
    assert sc[16 - 8, 16 + 3] == g[CY - 8, 75]                 # dy = -8 is row 64: still outside
    assert sc[0, 0] == g[CY - 16, 56] + g[56, CX - 16]


def test_spoiled_ranges_and_gated_people_do_not_vote(rules):
    a, b = rules["spoiled"]
    # max_range = 2: of (0, 2, -1, 2, NaN, 1, 2, 2, 0) only beam 5 votes; of (inf, NaN, 0, -1, 2, 2.5, 1, 1.5, inf) beams 6, 7
    assert a["votes"] == 1 and b["votes"] == 2
    assert (a["cells"][4][:, 0] > -2 ** 40).tolist() == [False] * 5 + [True] + [False] * 3
    gate = rules["gate"][0]
    # beam 4 is row 0's (score 0.9): no vote; beam 6 is row 1's (0.2, under cls_thresh): votes; ids 5 and -1 are nobody's
    assert gate["votes"] == 3 and gate["cells"][4][4, 0] == -2 ** 40 and tuple(gate["cells"][4][6]) == (CX, 40)
    first, second = rules["clamped"]
    # num_det = 100 counts as N = 9: id 9 is row 8 (a person), id 10 nobody's; num_det = -3 counts as 0
    assert first["votes"] == 3 and first["cells"][4][4, 0] == -2 ** 40 and second["votes"] == 4


def test_the_gates_flip_exactly_at_equality(rules):
    at, few, low, gain = (rules[k][0] for k in ("ok at equality", "too few points", "score too low", "gain too low"))
    for o in (at, few, low, gain):
        assert o["votes"] == 4 and o["score"].tolist() == [120, 0] and o["best"].tolist() == [0, 0, 1]
    assert (at["ok"], at["moved"]) == (1, 1) and at["pose"][0] == 0.1875
    assert (few["ok"], few["moved"]) == (0, 0) and (low["ok"], low["moved"]) == (0, 0)
    assert (gain["ok"], gain["moved"]) == (1, 0)
    pose = RULE_POSE.copy()
    for o in (few, low, gain):                                 # without moved: the same bits, zeros as the correction
        assert o["pose"].tobytes() == pose.tobytes() and o["trans"].tobytes() == pose[:2].tobytes()
        assert o["rot"].tolist() == [1.0, 0.0, 0.0, 1.0] and not o["correction"].any()
    empty = rules["empty grid"][0]
    # an empty grid scores 0 everywhere: the zero candidate wins every tie, and even with every gate at 0 nothing moves
    assert not empty["scores"].any() and empty["best"].tolist() == [0, 0, 0] and (empty["ok"], empty["moved"]) == (1, 0)


def test_quarter_turn_pose_and_rotated_rows(rules):
    case = rule_cases()["quarter turn"]
    s, o = case["sensors"][0], rules["quarter turn"][0]
    mid = o["cells"][4]
    assert tuple(mid[4]) == (CX, 40) and tuple(mid[6]) == (56, CY)             # tests/test_grid_map.py's quarter turn
    # the rows beside the middle one really turn the scan: beam 5 (2.5 m out) moves by 0.04 rad x 2.5 m = a cell
    assert not np.array_equal(o["cells"][0], o["cells"][8]) and o["votes"] == 4
    if o["moved"]:
        k = o["best"][0]
        assert o["pose"][2] == np.pi / 2 + rotation_table(0.01, 9)[4 + k, 0]
        assert np.array_equal(o["rot"], pose_terms(o["pose"])[0])


# ---------------------------------------------------------------- rooms: the cases the device is held to
def room_case(seed, N, H, W, sensors=1, scans=5, people=True, offsets=((0.0, 0.0, 0.0),), res=0.1, **kw):
    """tests/test_grid_map.room_scene's sensors: the map of each from its first scans at their true poses
    (``grid_map_oracle``), its last scan matched at the true pose moved by offsets[b % len(offsets)]."""
    scene = room_scene(seed, scans, N, H, W, res=res, sensors=sensors, people=people)
    out = []
    for b, sensor in enumerate(scene["sensors"]):
        grid = np.zeros((H, W), np.int16)
        for s in sensor["scans"][:-1]:
            grid_map_oracle(s["ranges"], scene["tab"], s["rot"], s["trans"], grid, sensor["origin"], res, s.get("inst"),
                            s.get("num_det"), s.get("det_cls"), **scene["kw"])
        last = sensor["scans"][-1]
        phi = float(np.arctan2(np.float64(last["rot"][1, 0]), np.float64(last["rot"][0, 0])))
        pose = np.array([last["trans"][0], last["trans"][1], phi]) + np.asarray(offsets[b % len(offsets)], np.float64)
        rot, trans = pose_terms(pose)
        s = dict(ranges=last["ranges"], rot=rot.reshape(2, 2), trans=trans, pose=pose, grid=grid,
                 origin=np.asarray(sensor["origin"], np.float64))
        if people:
            s.update(inst=last["inst"], num_det=last["num_det"], det_cls=last["det_cls"])
        out.append(s)
    return dict(tab=scene["tab"], H=H, W=W, res=res, kw=dict(DEFAULTS, **kw), sensors=out)


OFF = ((0.23, -0.17, 0.021), (0.0, 0.0, 0.0), (-0.31, 0.12, -0.03))


def device_cases():
    """-> {name: case}: the shapes tests/test_grid_match_gpu.py runs."""
    return {
        "one tile": room_case(52, 64, 64, 64, offsets=OFF[:1], min_points=5, min_score=10, max_range=6.0),
        "128 x 192 with people": room_case(53, 450, 128, 192, sensors=3, offsets=OFF),
        "N 512": room_case(54, 512, 128, 128, offsets=OFF[2:]),
        "N 513": room_case(55, 513, 128, 128, offsets=OFF[:1]),
        "N 4096": room_case(56, 4096, 64, 128, scans=3, offsets=OFF[:1], reach=1, rotations=3),
        "largest search": room_case(57, 64, 128, 128, offsets=((1.1, -0.9, 0.1),), reach=16, rotations=33, min_points=10,
                                    min_score=10, min_gain=5),
        "smallest search": room_case(58, 64, 128, 128, offsets=OFF[:1], reach=0, rotations=1, min_points=10),
        "no NMS": room_case(59, 450, 128, 128, people=False, offsets=OFF[2:]),
        # 3.2 m of grid around a sensor that sees 4 to 8 m: most of the scan ends outside, some of it within reach
        "leaves the grid": room_case(60, 450, 64, 64, sensors=2, offsets=OFF[:2], reach=8, min_points=10, min_score=5,
                                     min_gain=4),
    }


def test_device_cases_reach_their_shapes():
    cases = device_cases()
    got = {k: run_case(c) for k, c in cases.items() if k != "N 4096"}
    people = got["128 x 192 with people"]
    assert [int(o["moved"]) for o in people] == [1, 0, 1]       # the sensor at its true pose is left alone
    for o, off in zip(people, OFF):
        left = np.asarray(off) + o["correction"]
        assert np.abs(left[:2]).max() <= 0.1 and abs(left[2]) <= 0.015, left
    case = cases["128 x 192 with people"]
    s = case["sensors"][0]
    assert people[0]["votes"] < voting_points(s["ranges"]).sum()               # somebody is gated
    assert got["largest search"][0]["scores"].shape == (33, 33, 33) and got["largest search"][0]["moved"]
    assert np.abs(got["largest search"][0]["best"][1:]).max() > 8
    assert got["smallest search"][0]["scores"].shape == (1, 1, 1) and "inst" not in cases["no NMS"]["sensors"][0]
    away = cases["leaves the grid"]
    for s, o in zip(away["sensors"], got["leaves the grid"]):
        cells = o["cells"][4]
        voted = cells[:, 0] > -2 ** 40
        outside = voted & ((cells[:, 0] < 0) | (cells[:, 0] >= 64) | (cells[:, 1] < 0) | (cells[:, 1] >= 64))
        near = outside & (cells[:, 0] >= -8) & (cells[:, 0] < 72) & (cells[:, 1] >= -8) & (cells[:, 1] < 72)
        assert outside.sum() > 50 and near.sum() > 0, (outside.sum(), near.sum())
    assert len(cases["N 4096"]["sensors"][0]["ranges"]) == 4096 and any(o["moved"] for os_ in got.values() for o in os_)


# ---------------------------------------------------------------- what the stage is good for
QUALITY_SEEDS = (11, 12, 13, 14)
GRID, CELL, SCANS, SPOILED = 256, 0.1, 16, 13


def drive(seed, spoil=True):
    """One sensor driven through the middle of a room of its own (tests/test_scan_match.make_room keeps its boxes away
    from there), 0.105 to 0.115 m and 0.005 to 0.015 rad per scan: -> (tab, scans float32 [SCANS, 450] with 1 cm noise
    and a 225 degree view, scan SPOILED all NaN when ``spoil``, the true poses [SCANS, 3]).  Two lost pairs are at
    least 0.21 m and at most 0.03 rad: inside the default search of 0.4 m and 0.04 rad."""
    rng = np.random.default_rng(seed)
    N = 450
    tab = angle_table(N, np.radians(225.0) / N)
    segs = make_room(rng)
    phi = rng.uniform(-np.pi, np.pi)
    pose = np.array([-0.85 * np.cos(phi) + rng.uniform(-0.1, 0.1), -0.85 * np.sin(phi) + rng.uniform(-0.1, 0.1), phi])
    turn = rng.choice([-1.0, 1.0])
    scans, poses = np.zeros((SCANS, N), np.float32), np.zeros((SCANS, 3))
    for t in range(SCANS):
        poses[t] = pose
        scans[t] = (ray_cast(segs, pose, tab[:N]) + rng.normal(0.0, 1.0, N) * 0.01).astype(np.float32)
        step = rng.uniform(0.105, 0.115)
        pose = pose + np.array([step * np.cos(pose[2]), step * np.sin(pose[2]), turn * rng.uniform(0.005, 0.015)])
    if spoil:
        scans[SPOILED] = np.nan
    return tab, scans, poses


def advance(pose, motion):
    """pof_pose_advance: phi += theta, t += R(phi) u."""
    c, s = np.cos(pose[2]), np.sin(pose[2])
    return np.array([pose[0] + (c * motion[1] - s * motion[2]), pose[1] + (s * motion[1] + c * motion[2]),
                     pose[2] + motion[0]])


def reckon(tab, scans, start, matched, true_poses=None, size=GRID, **kw):
    """The streaming chain in float64: the scan match and the pose launch, then -- with ``matched`` -- the grid match,
    then the grid update at the resulting pose.  ``true_poses``: no scan match, the map is driven at these poses.
    -> (poses [T,3], the grid-match dicts or None per scan, the grid, the last scan's grid-map outputs)."""
    pose, init = np.asarray(start, np.float64).copy(), None
    origin = pose[:2] - 0.5 * CELL * size
    grid, poses, outs, last = np.zeros((size, size), np.int16), [], [], None
    for t, scan in enumerate(scans):
        if true_poses is not None:
            pose = true_poses[t].copy()
        elif t > 0:
            m = match_oracle(scans[t - 1], scan, tab, init=init)
            init = m["motion"]
            if m["ok"]:
                pose = advance(pose, m["motion"])
        rot, trans = pose_terms(pose)
        o = None
        if matched:
            o = grid_match_oracle(scan, tab, rot, trans, pose, grid, origin, CELL, **dict(DEFAULTS, **kw))
            pose, rot, trans = o["pose"], o["rot"], o["trans"]
        last = grid_map_oracle(scan, tab, rot, trans, grid, origin, CELL)
        poses.append(pose.copy())
        outs.append(o)
    return np.array(poses), outs, grid, last


@pytest.fixture(scope="module")
def driven():
    res = {}
    for seed in QUALITY_SEEDS:
        tab, scans, truth = drive(seed)
        clean = drive(seed, spoil=False)[1]
        res[seed] = dict(truth=truth, with_match=reckon(tab, scans, truth[0], True),
                         without=reckon(tab, scans, truth[0], False), undisturbed=reckon(tab, clean, truth[0], False))
    return res


def test_silence_at_true_poses():
    """(i) The map driven at the true poses: ``moved`` is False in every scan of every seed (cap 0), and from the fourth
    scan on the zero candidate is the best one and ``ok``.  Measured, seeds 11-14: score per voting point at the zero
    candidate 45.5-69.7 from the fourth scan on (14-16, 28-32 at the second and third), and no candidate above it in any
    scan."""
    for seed in QUALITY_SEEDS:
        tab, scans, truth = drive(seed, spoil=False)
        _, outs, _, _ = reckon(tab, scans, truth[0], True, true_poses=truth)
        per_point = [o["score"][1] / max(int(o["votes"]), 1) for o in outs]
        print("seed %d: zero candidate's score per voting point %s" % (seed, np.round(per_point, 1).tolist()))
        assert not any(o["moved"] for o in outs), seed
        assert all(o["best"].tolist() == [0, 0, 0] for o in outs[3:]), seed
        assert all(o["ok"] for o in outs[3:]) and not outs[0]["ok"]            # an empty grid: not ok


def test_recovery_after_a_spoiled_scan(driven):
    """(ii) Dead reckoning through ``match_oracle``; scan 13 is all NaN, so pairs (12, 13) and (13, 14) fail and about
    0.22 m of motion are lost.  The position error at the last scan with the stage is smaller than without it in every
    seed, and at most one cell diagonal above the error of the undisturbed sequence.  Measured, seeds 11-14: lost motion
    0.219-0.225 m; end error without 0.219-0.223 m, with 0.006-0.040 m, undisturbed 0.001-0.005 m; ``moved`` fires at
    scan 14, the first good scan behind the lost pairs, and at no other scan, in every seed."""
    for seed, d in driven.items():
        truth = d["truth"]
        err = {k: float(np.hypot(*(d[k][0][-1, :2] - truth[-1, :2]))) for k in ("with_match", "without", "undisturbed")}
        lost = float(np.hypot(*(truth[SPOILED + 1, :2] - truth[SPOILED - 1, :2])))
        fired = [t for t, o in enumerate(d["with_match"][1]) if o["moved"]]
        print("seed %d: lost %.3f m; end error without %.3f m, with %.3f m, undisturbed %.3f m; moved at scans %s"
              % (seed, lost, err["without"], err["with_match"], err["undisturbed"], fired))
        assert lost >= 2 * CELL
        assert err["with_match"] < err["without"], seed
        assert err["with_match"] <= np.sqrt(2.0) * CELL + err["undisturbed"], seed
        assert fired == [SPOILED + 1] and not d["with_match"][1][SPOILED]["ok"]   # a NaN scan has no votes


def test_map_health_after_the_sequence(driven):
    """(iii) The last scan's wall points on cells the map holds as free (<= -free_thresh) before that scan: fewer with
    the stage than without.  Measured, seeds 11-14: without 191-350 of 450 points, with 0-2."""
    for seed, d in driven.items():
        free = {}
        for k in ("with_match", "without"):
            last = d[k][3]
            free[k] = int(((last["point_cell"] >= 0) & (last["point_prior"].astype(np.int64) <= -MAP_DEFAULTS["free_thresh"])).sum())
        print("seed %d: wall points on free cells without %d, with %d" % (seed, free["without"], free["with_match"]))
        assert free["with_match"] < free["without"], seed


# ---------------------------------------------------------------- surface
def test_header_binding_and_wrappers():
    import torch
    from planar_optical_flow_amd import _lib, ops, streaming
    from planar_optical_flow_amd.src.utils import utils
    from planar_optical_flow_amd.streaming import StreamingDetector
    text = open(os.path.join(REPO, "include", "pof_abi.h")).read()
    m = re.search(r"\bint\s+pof_grid_match\s*\(([^)]*)\)\s*;", text)
    assert m, "include/pof_abi.h does not declare pof_grid_match"
    params = [p.strip() for p in m.group(1).split(",")]
    restype, argtypes = _lib.SIGNATURES["pof_grid_match"]
    assert restype is _lib._i and len(argtypes) == len(params) == 31
    for p, t in zip(params, argtypes):
        want = _lib._p if "*" in p or p.startswith("pof_stream_t") else _lib._d if p.startswith("double") else _lib._i
        assert t is want, p
    assert "N13" in text and "rot_tab" in text and "#define POF_ABI_VERSION 1" in text
    assert ops.GridMatch._fields == OUT_FIELDS
    rec = ops.grid_match_buffers(2, 3, 5, device="cpu")
    assert type(rec) is ops.GridMatch and [tuple(t.shape) for t in rec] == [(2, 5, 7, 7), (2, 3), (2, 2), (2,), (2,), (2,), (2, 3)]
    assert [t.dtype for t in rec] == [torch.int32] * 4 + [torch.uint8] * 2 + [torch.float64] and not any(t.any() for t in rec)
    for K, step in ((9, 0.01), (1, 0.3), (33, 0.005)):
        assert np.array_equal(ops.grid_match_table(step, K, device="cpu").numpy(), rotation_table(step, K))
    p = inspect.signature(ops.grid_match).parameters
    assert list(p)[:6] == ["ranges", "tab", "rot", "trans", "pose", "state"]
    assert {k: p[k].default for k in DEFAULTS} == DEFAULTS and p["res"].kind is inspect.Parameter.KEYWORD_ONLY
    assert p["table"].default is None and p["out"].default is None
    assert ops.stage_settings(ops.grid_match) == dict(DEFAULTS, res=ops.REQUIRED)
    want = {k: v for k, v in DEFAULTS.items() if k != "cls_thresh"}
    assert streaming.stage_defaults("grid_match") == want and streaming.stage_settings("grid_match", {}) == want
    assert streaming.stage_settings("grid_match", dict(reach=6)) == dict(want, reach=6)
    for unknown in ("cls_thresh", "res", "size"):
        with pytest.raises(ValueError, match="unknown grid_match settings"):
            streaming.stage_settings("grid_match", {unknown: 1})
    assert list(inspect.signature(utils.OccupancyGrid.localize).parameters)[1:] == ["scan", "odom", "pred_cls", "pred_reg",
                                                                                    "settings"]
    assert inspect.signature(StreamingDetector.__init__).parameters["grid_match"].default is None
    assert callable(StreamingDetector.grid_match)
    for bad in (dict(reach=17), dict(reach=-1), dict(rotations=8), dict(rotations=35), dict(rotations=0)):
        with pytest.raises(ValueError):
            ops.grid_match_buffers(1, **dict(dict(reach=4, rotations=9), **bad), device="cpu")
    # no CPU path
    f64 = torch.float64
    state = ops.GridMapState(torch.zeros(1, 64, 64, dtype=torch.int16), torch.zeros(1, 2, dtype=f64))
    with pytest.raises(TypeError):
        ops.grid_match(torch.zeros(1, 4), torch.zeros(12, dtype=f64), torch.zeros(1, 2, 2), torch.zeros(1, 2, dtype=f64),
                       torch.zeros(1, 3, dtype=f64), state, res=0.1)
    with pytest.raises(TypeError):
        ops.grid_match(None, None, None, None, None, None, res=0.1)


def test_entry_point_refuses_null_and_bad_arguments():
    import ctypes
    from planar_optical_flow_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "pof_grid_match")
    _, argtypes = _lib.SIGNATURES["pof_grid_match"]
    assert lib.pof_grid_match(*[None if t is _lib._p else 0 for t in argtypes]) == _lib.POF_E_BADARG
    assert lib.pof_grid_match(*[None if t is _lib._p else 1 for t in argtypes]) == _lib.POF_E_BADARG
    # every pointer given (never read: a refusal comes before any launch) and one bad setting at a time
    buf = ctypes.create_string_buffer(64)
    good = dict(cls_thresh=0.5, max_range=20.0, res=0.1, reach=4, rotations=9, min_points=50, min_score=20, min_gain=8,
                B=1, N=64, H=64, W=64)

    def call(nms=(1, 1, 1), **kw):
        v = dict(good, **kw)
        ptr = ctypes.addressof(buf)
        return lib.pof_grid_match(ptr, ptr, *[ptr if g else None for g in nms], v["cls_thresh"], v["max_range"], ptr, ptr,
                                  v["res"], ptr, v["reach"], v["rotations"], v["min_points"], v["min_score"],
                                  v["min_gain"], v["B"], v["N"], v["H"], v["W"], *[ptr] * 10, None)

    for bad in (dict(res=0.0), dict(res=float("nan")), dict(max_range=0.0), dict(reach=-1), dict(reach=17),
                dict(rotations=0), dict(rotations=8), dict(rotations=35), dict(min_points=-1), dict(min_score=-1),
                dict(min_gain=-1), dict(B=-1), dict(N=0)):
        assert call(**bad) == _lib.POF_E_BADARG, bad
    for nms in ((1, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert call(nms=nms) == _lib.POF_E_BADARG, nms
    for bad in (dict(N=4097), dict(H=96), dict(W=32), dict(H=2112), dict(W=100)):
        assert call(**bad) == _lib.POF_E_SHAPE, bad
    assert call(B=0) == _lib.POF_OK and call(B=0, nms=(0, 0, 0)) == _lib.POF_OK
