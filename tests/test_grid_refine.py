"""Grid refine (pof_grid_refine, N19) without a GPU: ``grid_refine_oracle`` is the float64 NumPy restatement of the
comment in include/pof_abi.h -- a Gauss-Newton fit of the scan endpoints to the bilinearly interpolated occupancy grid
of N12 -- checked here rule by rule on hand-painted grids whose numbers are exact, with four of its rules turned round to
show that a scene notices, and on ray-cast rooms for what the stage is good for: a pose that is tied to the map instead
of composed from scan pairs.  tests/test_grid_refine_gpu.py imports the restatement and the cases.

The eleven sums are restated in the device's own order (``group_sum``: thread i % THREADS adds its points in ascending
index, a butterfly over the 64 lanes of a wave, the waves in wave order), so the restatement and the device differ only
in the last bit of the one sincos per evaluation: at phi = 0 they agree bit for bit, elsewhere within the tolerance of
the ICP tests (1e-10, tests/test_scan_match_gpu.py).  The discrete decisions (s1 > s0, the exit, the shift and turn
gates, the pivots, the cell a point falls into) come with the margin by which they were taken (``margins``), and the
cases the device runs are asserted to keep every one >= 1e-10.

Quality, measured with this restatement (``circle``: rooms of tests/test_scan_match.make_room turned 0.3 rad against
the grid axes, the sensor on a circle of 1 m radius at 0.1 m per scan with tangent heading, 225 degree view, 450 beams,
1 cm range noise, 256 x 256 cells of 0.1 m, 252 scans = four laps): see the docstrings of the three quality tests, which
print their figures, and DESIGN.md 8 N19, which records them.  Three seeds (1-3) instead of the prototype's six keep the
module's quality fixtures under a minute."""
import inspect
import os
import re

import numpy as np
import pytest

from test_grid_map import grid_map_oracle
from test_grid_match import (CELL, GRID, SPOILED, advance, drive, grid_match_oracle, pose_terms, voting_points,
                             DEFAULTS as MATCH_DEFAULTS)
from test_scan_match import angle_table, make_room, match_oracle, ray_cast

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = dict(cls_thresh=0.5, max_range=20.0, cap=32, iters=8, min_points=50, min_pivot=1e-6, max_shift=2.0,
                max_turn=0.05, eps_shift=1e-3, eps_turn=1e-5)
OUT_FIELDS = ("correction", "score", "obs", "votes", "count", "iters_used", "ok", "moved")
OUT_DTYPES = (np.float64, np.float64, np.float64, np.int32, np.int32, np.int32, np.uint8, np.uint8)
EXACT, FLOATS = ("votes", "count", "iters_used", "ok", "moved"), ("correction", "score", "obs", "pose", "trans")
MARGIN_MIN = TOL = 1e-10
MUTATIONS = ("gain_ge", "no_half_cell", "no_clamp", "shift_lt")


# ---------------------------------------------------------------- restatement of the device arithmetic, one sensor
def group_sum(values, index, N):
    """The K sums of values [n,K] over the points ``index`` [n] of a scan of N points in the order of the device:
    point i belongs to thread i % THREADS (64 up to N = 512, else 512), which adds its points in ascending i from 0.0;
    a wave's 64 lanes meet in an xor butterfly (32, 16, ..., 1); the waves are added in wave order."""
    threads = 64 if N <= 512 else 512
    values, index = np.asarray(values, np.float64), np.asarray(index, np.int64)
    lanes = np.zeros((threads, values.shape[1]))
    for slot in range(8):
        of = index // threads == slot
        lanes[index[of] % threads] += values[of]               # one point per thread and slot: a plain add
    w = lanes.reshape(-1, 64, values.shape[1])
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, np.arange(64) ^ o]
    total = w[0, 0]
    for j in range(1, len(w)):
        total = total + w[j, 0]
    return total


def evaluate(px, py, votes, x, y, phi, grid, origin, res, cap, mutate=()):
    """The eleven sums at (x, y, phi) -> (S [11], inside [N] bool, the smallest distance of a voting point's (u, v)
    from a whole number)."""
    H, W = grid.shape
    N = len(px)
    s, c = np.sin(phi), np.cos(phi)
    half = 0.0 if "no_half_cell" in mutate else 0.5
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = c * px - s * py, s * px + c * py
        u, v = ((dx + x) - float(origin[0])) / res - half, ((dy + y) - float(origin[1])) / res - half
        i0, j0 = np.floor(u), np.floor(v)
        inside = votes & (i0 >= -1.0) & (i0 < W) & (j0 >= -1.0) & (j0 < H)
        fx, fy = (u - i0)[inside], (v - j0)[inside]
        near = np.minimum(np.abs(u - np.rint(u)), np.abs(v - np.rint(v)))[votes & np.isfinite(u) & np.isfinite(v)]
    ii, jj = i0[inside].astype(np.int64), j0[inside].astype(np.int64)
    cells = grid.astype(np.int64) if "no_clamp" in mutate else np.clip(grid.astype(np.int64), -cap, cap)
    m = np.zeros((H + 2, W + 2))
    m[1:-1, 1:-1] = cells.astype(np.float64) / float(cap)       # a cell outside the grid reads 0
    m00, m10, m01, m11 = m[jj + 1, ii + 1], m[jj + 1, ii + 2], m[jj + 2, ii + 1], m[jj + 2, ii + 2]
    M = (m00 * (1.0 - fx) + m10 * fx) * (1.0 - fy) + (m01 * (1.0 - fx) + m11 * fx) * fy
    gx = (m10 - m00) * (1.0 - fy) + (m11 - m01) * fy
    gy = (m01 - m00) * (1.0 - fx) + (m11 - m10) * fx
    lx, ly = dx[inside] / res, dy[inside] / res
    J = (gx, gy, gy * lx - gx * ly)
    e = 1.0 - M
    cols = [J[a] * J[b] for a in range(3) for b in range(a, 3)] + [J[a] * e for a in range(3)] + [M, np.ones_like(M)]
    return group_sum(np.stack(cols, axis=1), np.flatnonzero(inside), N), inside, float(near.min(initial=np.inf))


def grid_refine_oracle(ranges, tab, pose, grid, origin, res, inst=None, num_det=None, det_cls=None, rot=None,
                       trans=None, cls_thresh=0.5, max_range=20.0, cap=32, iters=8, min_points=50, min_pivot=1e-6,
                       max_shift=2.0, max_turn=0.05, eps_shift=1e-3, eps_turn=1e-5, mutate=()):
    """One scan of one sensor against its grid [H,W] int16 (read only).  ranges [N] float32, tab [3N], pose [3]; inst
    [N], num_det, det_cls [N] padded like the NMS outputs, all three or none; rot float32 [4] and trans [2]: the
    incoming pose terms, which come back untouched without ``moved`` (None: those of the pose).  ``mutate``: names of
    MUTATIONS, rules turned round.  -> dict of the eight outputs, the new pose, rot [4] float32 and trans, ``inside``
    [N] bool at the incoming pose, and margins {kind: the smallest margin of a decision of that kind}."""
    r = np.asarray(ranges, np.float32).astype(np.float64)
    N = len(r)
    tab = np.asarray(tab, np.float64)
    pose = np.asarray(pose, np.float64).copy()
    votes = voting_points(ranges, inst, num_det, det_cls, cls_thresh, max_range)
    V = int(votes.sum())
    with np.errstate(invalid="ignore", over="ignore"):
        px, py = r * tab[N::2], r * tab[N + 1::2]
    c = np.zeros(3)
    ok, last, used, obs, count, s0, s1, first_inside = V >= int(min_points), False, 0, 0.0, 0, np.nan, np.nan, None
    margins = {}

    def took(kind, value):
        if np.isfinite(value):
            margins[kind] = min(margins.get(kind, np.inf), float(value))

    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        while True:
            S, inside, near = evaluate(px, py, votes, pose[0] + c[0] * res, pose[1] + c[1] * res, pose[2] + c[2], grid,
                                       origin, res, int(cap), mutate)
            took("cell", near)
            n = int(S[10])
            if first_inside is None:
                first_inside, count, s0 = inside, n, S[9] / S[10]
            if n < int(min_points):
                ok = False
            if not ok:
                break
            if last:
                s1 = S[9] / S[10]
                break
            A00, A01, A02, A11, A12, A22, b0, b1, b2 = S[:9]
            dmax = max(A00, max(A11, A22))
            floor_ = min_pivot * dmax
            pivots = [A00]
            ok = bool(pivots[0] > floor_)
            if ok:
                l00 = np.sqrt(pivots[0])
                l10, l20 = A01 / l00, A02 / l00
                pivots.append(A11 - l10 * l10)
                ok = bool(pivots[1] > floor_)
                if ok:
                    l11 = np.sqrt(pivots[1])
                    l21 = (A12 - l20 * l10) / l11
                    pivots.append((A22 - l20 * l20) - l21 * l21)
                    ok = bool(pivots[2] > floor_)
                    if ok:
                        l22 = np.sqrt(pivots[2])
            obs = float(min(pivots) / dmax) if dmax > 0.0 else 0.0
            if dmax > 0.0:
                for p in pivots:
                    took("pivot", abs(p / dmax - min_pivot))
            if not ok:
                break
            y0 = b0 / l00
            y1 = (b1 - l10 * y0) / l11
            y2 = ((b2 - l20 * y0) - l21 * y1) / l22
            x2 = y2 / l22
            x1 = (y1 - l21 * x2) / l11
            x0 = ((y0 - l10 * x1) - l20 * x2) / l00
            c = c + np.array([x0, x1, x2])
            used += 1
            shift, turn = max(abs(x0), abs(x1)), abs(x2)
            took("stop", min(abs(shift - eps_shift), abs(turn - eps_turn)))
            last = used == int(iters) or (shift < eps_shift and turn < eps_turn)
    reach = max(abs(c[0]), abs(c[1]))
    moved = bool(ok and (reach < max_shift if "shift_lt" in mutate else reach <= max_shift) and abs(c[2]) <= max_turn
                 and (s1 >= s0 if "gain_ge" in mutate else s1 > s0))
    if ok:
        took("gain", abs(s1 - s0))
        took("shift", abs(reach - max_shift))
        took("turn", abs(abs(c[2]) - max_turn))
    rot4, trans2 = pose_terms(pose)
    rot4 = rot4 if rot is None else np.asarray(rot, np.float32).reshape(4).copy()
    trans2 = trans2 if trans is None else np.asarray(trans, np.float64).copy()
    correction = np.zeros(3)
    if moved:
        correction = np.array([c[0] * res, c[1] * res, c[2]])
        pose = np.array([pose[0] + c[0] * res, pose[1] + c[1] * res, pose[2] + c[2]])
        rot4, trans2 = pose_terms(pose)
    return dict(correction=correction, score=np.array([s0, s1 if ok else np.nan]), obs=float(obs), votes=np.int32(V),
                count=np.int32(count), iters_used=np.int32(used), ok=np.uint8(ok), moved=np.uint8(moved), pose=pose,
                rot=rot4, trans=trans2, inside=first_inside, margins=margins, cells=c)


def run_case(case, mutate=()):
    """The restatement over every sensor of a case -> list of its dicts."""
    return [grid_refine_oracle(s["ranges"], case["tab"], s["pose"], s["grid"], s["origin"], case["res"], s.get("inst"),
                               s.get("num_det"), s.get("det_cls"), mutate=mutate, **case["kw"]) for s in case["sensors"]]


def smallest_margins(results):
    out = {}
    for o in results:
        for k, v in o["margins"].items():
            out[k] = min(out.get(k, np.inf), v)
    return out


# ---------------------------------------------------------------- rule scenes: exact numbers
# 64 x 64 cells of 1/8 m around the world origin; cell (ix, iy) has its centre at ((ix + 0.5) / 8 - 4, (iy + 0.5) / 8 - 4).
# The table of a rule scene holds the points themselves as its (cos, sin) pairs and every voting range is 1: the launch
# only ever multiplies the two, so the endpoints, and with them every cell coordinate, are dyadic numbers.
RES, SIDE = 0.125, 64
ORIGIN = np.array([-4.0, -4.0])
WALL = 48                                                      # the painted column and row
LINE = (20, 28, 36, 44)


def centre_of(ix, iy):
    return ((ix + 0.5) * RES - 4.0, (iy + 0.5) * RES - 4.0)


def points_table(points):
    """[3N]: N zeros for the angles (never read by the stage) and the points as the (cos, sin) pairs."""
    pts = np.asarray(points, np.float64)
    return np.concatenate([np.zeros(len(pts)), pts.reshape(-1)])


def corner_grid(value=32):
    """Column WALL painted below row WALL, row WALL painted left of and at column WALL: two walls that meet."""
    g = np.zeros((SIDE, SIDE), np.int16)
    g[:WALL, WALL] = value
    g[WALL, :WALL + 1] = value
    return g


CORNER = [centre_of(WALL, j) for j in LINE] + [centre_of(i, WALL) for i in LINE]      # four points on either wall
ONE_WALL = [centre_of(WALL, j) for j in (8, 12, 16, 20, 24, 28, 32, 36)]
ONES = (1.0,) * 8
GATED = dict(inst=(1, 0, 2, 0, 0, 9, -1, 0), num_det=2, det_cls=(0.9, 0.2))


def _sensor(grid, pose=(0.0, 0.0, 0.0), ranges=ONES, inst=None, num_det=None, det_cls=None):
    s = dict(ranges=np.asarray(ranges, np.float32), pose=np.asarray(pose, np.float64), grid=np.asarray(grid, np.int16),
             origin=ORIGIN.copy())
    if inst is not None:
        cls = np.zeros(len(s["ranges"]))
        cls[:len(det_cls)] = det_cls
        s.update(inst=np.asarray(inst, np.int32), num_det=np.int32(num_det), det_cls=cls)
    return s


def _case(kw, *sensors, points=CORNER):
    return dict(tab=points_table(points), H=SIDE, W=SIDE, res=RES, kw=dict(DEFAULTS, **kw), sensors=list(sensors))


QUARTER = 0.25 * RES                                           # a quarter cell in metres


def edge_points():
    """Eight points on row 32: u = -1.5 (i0 = -2: outside), -0.75 (i0 = -1), 0.25, 31, 62.5, 63.25 (i0 = W - 1), 64.5
    (i0 = W: outside) and 30."""
    return [((u + 0.5) * RES - 4.0, centre_of(0, 32)[1]) for u in (-1.5, -0.75, 0.25, 31.0, 62.5, 63.25, 64.5, 30.0)]


def rule_cases():
    """-> {name: case}; a case is dict(tab, H, W, res, kw, sensors=[dict(ranges, pose, grid, origin and the NMS
    results)]).  The tests below say what each is for."""
    few = dict(min_points=1)
    quarter_x, quarter_y = _sensor(corner_grid(), (QUARTER, 0.0, 0.0)), _sensor(corner_grid(), (0.0, QUARTER, 0.0))
    row = np.zeros((SIDE, SIDE), np.int16)
    row[32] = 32
    return {
        "empty grid": _case(dict(min_points=0), _sensor(np.zeros((SIDE, SIDE), np.int16))),
        "quarter cell in x": _case(few, quarter_x),
        "quarter cell in y": _case(few, quarter_y),
        "turned": _case(few, _sensor(corner_grid(), (0.0, 0.0, 0.004))),
        "edges": _case(few, _sensor(row), points=edge_points()),
        "cap below": _case(dict(few, cap=8), _sensor(corner_grid(16), (QUARTER, 0.0, 0.0))),
        "cap above": _case(dict(few, cap=64), _sensor(corner_grid(16), (QUARTER, 0.0, 0.0))),
        "points at the minimum": _case(dict(min_points=8), quarter_x),
        "one vote short": _case(dict(min_points=9), quarter_x),
        "one inside short": _case(dict(min_points=8), quarter_x,
                                  points=CORNER[:7] + [(centre_of(20, 0)[0], -4.0 - 3 * RES)]),
        "single wall": _case(few, _sensor(corner_grid(), (QUARTER, 0.0, 0.0)), points=ONE_WALL),
        "not better": _case(few, _sensor(corner_grid())),
        "spoiled": _case(few, _sensor(corner_grid(), (QUARTER, 0.0, 0.0),
                                      ranges=(1.0, np.nan, 1.0, np.inf, 1.0, 0.0, -1.0, 3.0))),
        "gate": _case(few, _sensor(corner_grid(), (QUARTER, 0.0, 0.0), **GATED)),
        "one iteration": _case(dict(few, iters=1), quarter_x),
        "one point": _case(few, _sensor(corner_grid(), (QUARTER, 0.0, 0.0), ranges=(1.0,)), points=CORNER[:1]),
    }


def gate_cases():
    """The shift and turn gates at the correction the restatement finds and one ulp under it."""
    x = run_case(rule_cases()["quarter cell in x"])[0]["cells"]
    t = run_case(rule_cases()["turned"])[0]["cells"]
    shift, turn = float(max(abs(x[0]), abs(x[1]))), float(abs(t[2]))
    few = dict(min_points=1)
    return {
        "shift at": _case(dict(few, max_shift=shift), _sensor(corner_grid(), (QUARTER, 0.0, 0.0))),
        "shift beyond": _case(dict(few, max_shift=float(np.nextafter(shift, 0.0))), _sensor(corner_grid(), (QUARTER, 0.0, 0.0))),
        "turn at": _case(dict(few, max_turn=turn), _sensor(corner_grid(), (0.0, 0.0, 0.004))),
        "turn beyond": _case(dict(few, max_turn=float(np.nextafter(turn, 0.0))), _sensor(corner_grid(), (0.0, 0.0, 0.004))),
    }


@pytest.fixture(scope="module")
def rules():
    return {k: run_case(c) for k, c in dict(rule_cases(), **gate_cases()).items()}


def test_group_sum_is_the_device_order():
    rng = np.random.default_rng(0)
    v = rng.normal(0, 1, (700, 2)) * 10.0 ** rng.integers(-8, 8, (700, 2))
    idx = np.sort(rng.choice(4096, 700, replace=False))
    for N in (4096,):
        got = group_sum(v, idx, N)
        lanes = [[0.0, 0.0] for _ in range(512)]
        for i, row in zip(idx, v):                             # ascending i: a thread's slots in slot order
            lanes[i % 512] = [lanes[i % 512][0] + row[0], lanes[i % 512][1] + row[1]]
        lanes = np.array(lanes).reshape(8, 64, 2)
        for o in (32, 16, 8, 4, 2, 1):
            lanes = np.array([[lanes[w, l] + lanes[w, l ^ o] for l in range(64)] for w in range(8)])
        assert (lanes == lanes[:, :1]).all()                   # every lane of a wave ends with the same bits
        want = lanes[0, 0]
        for w in range(1, 8):
            want = want + lanes[w, 0]
        assert got.tobytes() == want.tobytes()
    small = group_sum(v[:100], np.arange(100) * 5, 512)        # one wave: thread i % 64
    assert abs(small - v[:100].sum(axis=0)).max() <= 1e-9 * np.abs(v[:100]).sum()
    assert group_sum(np.zeros((0, 3)), np.zeros(0, int), 8).tolist() == [0.0, 0.0, 0.0]


def test_an_empty_grid_is_not_ok(rules):
    o = rules["empty grid"][0]
    assert (o["votes"], o["count"], o["iters_used"], o["ok"], o["moved"]) == (8, 8, 0, 0, 0)
    assert o["score"][0] == 0.0 and np.isnan(o["score"][1]) and o["obs"] == 0.0 and not o["correction"].any()
    assert o["pose"].tolist() == [0.0, 0.0, 0.0] and o["rot"].tolist() == [1.0, 0.0, 0.0, 1.0]


def test_a_wall_a_quarter_cell_off_is_put_back(rules):
    """The four points on the wall across the offset read M = 0.75 with gradient -1, the four on the other wall M = 1:
    s0 = 0.875, the first step is the quarter cell, the second finds nothing left and the third evaluation scores."""
    for name, axis in (("quarter cell in x", 0), ("quarter cell in y", 1)):
        o = rules[name][0]
        assert (o["votes"], o["count"], o["iters_used"], o["ok"], o["moved"]) == (8, 8, 2, 1, 1), name
        assert o["score"][0] == 0.875 and abs(o["score"][1] - 1.0) <= 1e-12
        want = np.zeros(3)
        want[axis] = -QUARTER
        assert np.abs(o["correction"] - want).max() <= 1e-12 and np.abs(o["pose"]).max() <= 1e-12
        assert np.array_equal(o["trans"], o["pose"][:2]) and np.array_equal(o["rot"], pose_terms(o["pose"])[0])
        assert o["obs"] > 1e-3


def test_two_walls_hold_a_small_rotation(rules):
    o = rules["turned"][0]
    assert (o["ok"], o["moved"]) == (1, 1) and 2 <= o["iters_used"] <= 8
    assert abs(o["pose"][2]) < 2e-4 and np.abs(o["pose"][:2]).max() < 0.02 * RES and o["score"][1] > o["score"][0]
    assert np.array_equal(o["rot"], pose_terms(o["pose"])[0])


def test_the_padded_neighbour_reads_zero_and_one_cell_beyond_is_outside(rules):
    o = rules["edges"][0]
    # u = -1.5 and 64.5 are outside; -0.75 reads 0.25 of column 0, 63.25 reads 0.75 of column 63, the others 1
    assert o["inside"].tolist() == [False, True, True, True, True, True, False, True] and o["count"] == 6
    assert o["votes"] == 8 and o["score"][0] == (0.25 + 1.0 + 1.0 + 1.0 + 0.75 + 1.0) / 6.0


def test_cap_below_and_above_the_cell_values(rules):
    below, above = rules["cap below"][0], rules["cap above"][0]
    assert below["score"][0] == 0.875                          # 16 clamped to 8: m = 1, as the corner at 32 / 32
    assert above["score"][0] == 0.25 * 0.875                   # 16 / 64
    assert below["ok"] and below["moved"] and abs(below["correction"][0] + QUARTER) <= 1e-12
    # at a quarter of the cap no point ever reaches e = 0: the fit walks off the walls and the pose is left alone
    assert not above["moved"] and above["pose"].tolist() == [QUARTER, 0.0, 0.0]


def test_votes_and_count_at_min_points_and_one_under(rules):
    at, votes, inside = (rules[k][0] for k in ("points at the minimum", "one vote short", "one inside short"))
    assert (at["votes"], at["count"], at["ok"], at["moved"]) == (8, 8, 1, 1)
    assert (votes["votes"], votes["count"], votes["ok"], votes["iters_used"]) == (8, 8, 0, 0)
    assert (inside["votes"], inside["count"], inside["ok"], inside["iters_used"]) == (8, 7, 0, 0)
    for o in (votes, inside):
        assert np.isnan(o["score"][1]) and o["pose"].tolist() == [QUARTER, 0.0, 0.0] and not o["correction"].any()


def test_a_single_wall_fails_a_pivot_and_leaves_the_pose(rules):
    o = rules["single wall"][0]
    assert (o["votes"], o["count"], o["ok"], o["moved"], o["iters_used"]) == (8, 8, 0, 0, 0)
    assert o["score"][0] == 0.75 and np.isnan(o["score"][1]) and o["obs"] == 0.0      # A11 = 0: nothing holds y
    assert o["pose"].tolist() == [QUARTER, 0.0, 0.0] and o["trans"].tolist() == [QUARTER, 0.0]
    one = rules["one point"][0]
    assert (one["votes"], one["count"], one["ok"], one["moved"]) == (1, 1, 0, 0)


def test_the_shift_and_turn_gates_hold_at_equality(rules):
    for at, beyond in (("shift at", "shift beyond"), ("turn at", "turn beyond")):
        a, b = rules[at][0], rules[beyond][0]
        assert (a["ok"], a["moved"], b["ok"], b["moved"]) == (1, 1, 1, 0), at
        assert np.array_equal(a["cells"], b["cells"]) and not b["correction"].any() and a["correction"].any()
        assert b["score"][1] > b["score"][0]                   # it is the gate that holds the pose, not the score


def test_a_pose_that_scores_no_better_is_not_moved(rules):
    o = rules["not better"][0]
    assert (o["ok"], o["moved"], o["iters_used"]) == (1, 0, 1) and o["score"].tolist() == [1.0, 1.0]
    assert not o["correction"].any() and o["pose"].tolist() == [0.0, 0.0, 0.0]


def test_spoiled_ranges_and_gated_people_do_not_vote(rules):
    spoiled, gate = rules["spoiled"][0], rules["gate"][0]
    # NaN, inf, 0, -1 do not vote; 3.0 votes and ends outside the corner's walls
    assert spoiled["votes"] == 4 and spoiled["inside"].tolist() == [True, False, True, False, True, False, False, False]
    # point 0 is row 0's (0.9): no vote; point 2 is row 1's (0.2): votes; ids 9 and -1 are nobody's
    assert gate["votes"] == 7 and gate["inside"].tolist() == [False] + [True] * 7
    assert gate["score"][0] == (3 * 0.75 + 4.0) / 7.0


def test_one_iteration_is_one_update_and_two_evaluations(rules):
    o = rules["one iteration"][0]
    assert (o["iters_used"], o["ok"], o["moved"]) == (1, 1, 1) and o["score"][0] == 0.875
    assert abs(o["score"][1] - 1.0) <= 1e-12 and abs(o["correction"][0] + QUARTER) <= 1e-12


def test_each_rule_turned_round_changes_a_named_scene(rules):
    cases = dict(rule_cases(), **gate_cases())
    hits = {"gain_ge": ("not better", "moved"), "no_half_cell": ("quarter cell in x", "score"),
            "no_clamp": ("cap below", "score"), "shift_lt": ("shift at", "moved")}
    assert set(hits) == set(MUTATIONS)
    for rule, (name, field) in hits.items():
        turned = run_case(cases[name], mutate=(rule,))[0]
        assert not np.array_equal(turned[field], rules[name][0][field], equal_nan=True), (rule, name)
    # and none of them is noticed where it should not matter
    assert run_case(cases["quarter cell in x"], mutate=("gain_ge", "shift_lt"))[0]["moved"] == 1


# ---------------------------------------------------------------- rooms: the cases the device is held to
def room_case(seed, N, H, W, sensors=1, scans=6, offsets=((0.02, -0.03, 0.004),), res=0.1, people=False, **kw):
    """tests/test_grid_map.room_scene's sensors: the map of each from its first scans at their true poses, its last scan
    refined from the true pose moved by offsets[b % len(offsets)]."""
    from test_grid_map import room_scene
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
        s = dict(ranges=last["ranges"], pose=pose, grid=grid, origin=np.asarray(sensor["origin"], np.float64))
        if people:
            s.update(inst=last["inst"], num_det=last["num_det"], det_cls=last["det_cls"])
        out.append(s)
    return dict(tab=scene["tab"], H=H, W=W, res=res, kw=dict(DEFAULTS, **kw), sensors=out)


OFF = ((0.02, -0.03, 0.004), (0.0, 0.0, 0.0), (-0.04, 0.01, -0.006))


def device_cases():
    """-> {name: case}: the room shapes tests/test_grid_refine_gpu.py runs beside the rule scenes."""
    return {
        "one tile": room_case(71, 64, 64, 64, res=0.25, min_points=10),
        "64 x 128 with people": room_case(72, 450, 64, 128, sensors=3, offsets=OFF, people=True, min_points=20),
        "N 512": room_case(73, 512, 128, 128, offsets=OFF[2:]),
        "N 513": room_case(74, 513, 128, 128),
        "N 4096": room_case(75, 4096, 128, 128, scans=3),
        "2048 x 64": room_case(76, 450, 2048, 64, min_points=10),
    }


def test_device_cases_reach_their_shapes_and_keep_their_margins():
    cases = device_cases()
    got = {k: run_case(c) for k, c in cases.items()}
    margins = smallest_margins([o for os_ in got.values() for o in os_])
    print("device cases: smallest margins %s" % {k: "%.2e" % v for k, v in sorted(margins.items())})
    assert all(v >= MARGIN_MIN for v in margins.values()), margins
    assert all(o["ok"] for os_ in got.values() for o in os_)
    people = got["64 x 128 with people"]
    for o, off in zip(people, OFF):
        left = np.asarray(off) + o["correction"]
        assert np.hypot(*left[:2]) <= 0.1 / np.sqrt(2.0), left
    s = cases["64 x 128 with people"]["sensors"][0]
    assert people[0]["votes"] < voting_points(s["ranges"]).sum()                # somebody is gated
    assert any(o["moved"] for o in people) and got["2048 x 64"][0]["count"] < got["2048 x 64"][0]["votes"]
    assert len(cases["N 4096"]["sensors"][0]["ranges"]) == 4096 and cases["2048 x 64"]["sensors"][0]["grid"].shape == (2048, 64)


def test_rule_scenes_keep_their_margins_where_a_sine_enters():
    """At phi = 0 the device's sincos is exact and the scenes hold bit for bit; the turned scenes need the margins."""
    cases = rule_cases()
    margins = smallest_margins(run_case(cases["turned"]))
    del margins["cell"]                                        # the painted walls are flat across a cell border
    assert all(v >= MARGIN_MIN for v in margins.values()), margins


# ---------------------------------------------------------------- what the stage is good for
QUALITY_SEEDS = (1, 2, 3)
LAPS, PER_LAP = 4, 63
TURN = 0.3


def circle(seed, scans=LAPS * PER_LAP):
    """One sensor on a circle of 1 m radius around the middle of a room of its own (tests/test_scan_match.make_room,
    turned TURN rad against the grid axes), 0.1 m per scan, heading along the tangent: -> (tab, scans float32 [T, 450]
    with 1 cm noise and a 225 degree view, the true poses [T, 3])."""
    rng = np.random.default_rng(seed)
    N = 450
    tab = angle_table(N, np.radians(225.0) / N)
    segs = make_room(rng)
    c, s = np.cos(TURN), np.sin(TURN)
    segs = np.stack([c * segs[..., 0] - s * segs[..., 1], s * segs[..., 0] + c * segs[..., 1]], axis=-1)
    a = 0.1 * np.arange(scans)
    poses = np.stack([np.cos(a), np.sin(a), a + np.pi / 2], axis=1)
    out = np.zeros((scans, N), np.float32)
    for t in range(scans):
        out[t] = (ray_cast(segs, poses[t], tab[:N]) + rng.normal(0.0, 1.0, N) * 0.01).astype(np.float32)
    return tab, out, poses


def localise(tab, scans, start, refine, matched=False, true_poses=None, size=GRID, **kw):
    """The streaming chain in float64: the scan match and the pose launch, then -- with ``matched`` -- the grid match,
    then -- with ``refine`` -- the refine, then the grid update at the resulting pose.  ``true_poses``: no scan match,
    the map is driven at these poses and the refined pose is reported but not used.
    -> (poses [T,3], the refine dicts or None per scan)."""
    pose, init = np.asarray(start, np.float64).copy(), None
    origin = pose[:2] - 0.5 * CELL * size
    grid, poses, outs = np.zeros((size, size), np.int16), [], []
    for t, scan in enumerate(scans):
        if true_poses is not None:
            pose = true_poses[t].copy()
        elif t > 0:
            m = match_oracle(scans[t - 1], scan, tab, init=init)
            init = m["motion"]
            if m["ok"]:
                pose = advance(pose, m["motion"])
        rot, trans = pose_terms(pose)
        if matched:
            o = grid_match_oracle(scan, tab, rot, trans, pose, grid, origin, CELL, **MATCH_DEFAULTS)
            pose, rot, trans = o["pose"], o["rot"], o["trans"]
        o, at = None, pose
        if refine:
            o = grid_refine_oracle(scan, tab, pose, grid, origin, CELL, **dict(DEFAULTS, **kw))
            at = o["pose"]
            if true_poses is None:
                pose = at
        rot, trans = pose_terms(pose)
        grid_map_oracle(scan, tab, rot, trans, grid, origin, CELL)
        poses.append(np.asarray(at, np.float64).copy())
        outs.append(o)
    return np.array(poses), outs


def position_error(poses, truth):
    return np.hypot(*(poses[:, :2] - truth[:, :2]).T)


@pytest.fixture(scope="module")
def laps():
    res = {}
    for seed in QUALITY_SEEDS:
        tab, scans, truth = circle(seed)
        res[seed] = dict(truth=truth, refined=localise(tab, scans, truth[0], True),
                         plain=localise(tab, scans, truth[0], False)[0],
                         at_truth=localise(tab, scans, truth[0], True, true_poses=truth))
    return res


def test_on_a_map_built_at_true_poses_the_refined_pose_stays_within_half_a_cell(laps):
    """(i) The map driven at the true poses, every scan refined from the true pose: the refined pose stays within
    res / sqrt(2) = 0.0707 m of truth at every scan -- the half-cell diagonal, the map's quantisation.  Measured, seeds
    1-3: the largest deviation over the run 0.0088-0.0105 m (heading 0.0019-0.0039 rad), 3.9-4.5 updates per scan on average,
    ``moved`` in 212-238 of 252 scans."""
    for seed, d in laps.items():
        poses, outs = d["at_truth"]
        err = position_error(poses, d["truth"])
        used = [int(o["iters_used"]) for o in outs]
        print("seed %d: refined from truth: max deviation %.4f m, heading %.4f rad, mean updates %.2f, moved in %d of %d"
              % (seed, err.max(), np.abs(poses[:, 2] - d["truth"][:, 2]).max(), np.mean(used),
                 sum(int(o["moved"]) for o in outs), len(outs)))
        assert err.max() <= CELL / np.sqrt(2.0), seed
        assert not outs[0]["ok"] and all(o["ok"] for o in outs[3:])             # an empty grid: not ok


def test_four_laps_end_nearer_to_truth_with_the_refine(laps):
    """(ii) Dead reckoning through ``match_oracle`` over four laps of the circle, with and without the refine behind the
    pose launch: per seed the end position error and the end heading error with the refine are below those without,
    and the position error with it never exceeds res / sqrt(2).  Measured, seeds 1-3: end position error without 0.013-0.044 m, with 0.006-0.011 m (0.018-0.020 m at most
    over the run); end heading error without 0.031-0.045 rad, with 0.002-0.007 rad; 3.5-3.9 updates per scan on average."""
    for seed, d in laps.items():
        truth = d["truth"]
        with_, without = d["refined"][0], d["plain"]
        e1, e0 = position_error(with_, truth), position_error(without, truth)
        h1, h0 = abs(with_[-1, 2] - truth[-1, 2]), abs(without[-1, 2] - truth[-1, 2])
        used = [int(o["iters_used"]) for o in d["refined"][1]]
        print("seed %d: end position error without %.4f m, with %.4f m (max over the run %.4f m); end heading error "
              "without %.4f rad, with %.4f rad; mean updates %.2f" % (seed, e0[-1], e1[-1], e1.max(), h0, h1, np.mean(used)))
        assert e1[-1] < e0[-1] and h1 < h0, seed
        assert e1.max() <= CELL / np.sqrt(2.0), seed


def test_behind_the_grid_match_a_lost_scan_pair_is_still_recovered():
    """(iii) tests/test_grid_match.drive with its spoiled scan, ``grid_match`` and then the refine: the end error is at
    most one cell diagonal above the undisturbed sequence's -- the bound N13's own test uses.  Measured, seeds 11-14:
    0.020-0.029 m with both stages, 0.001-0.005 m undisturbed."""
    for seed in (11, 12, 13, 14):
        tab, scans, truth = drive(seed)
        clean = drive(seed, spoil=False)[1]
        both = localise(tab, scans, truth[0], True, matched=True)[0]
        undisturbed = localise(tab, clean, truth[0], False)[0]
        e, u = position_error(both, truth)[-1], position_error(undisturbed, truth)[-1]
        print("seed %d: end error with grid_match and refine %.4f m, undisturbed without either %.4f m" % (seed, e, u))
        assert e <= np.sqrt(2.0) * CELL + u, seed
        assert SPOILED < len(scans)


# ---------------------------------------------------------------- surface
def test_header_binding_and_wrappers():
    import torch
    from planar_optical_flow_amd import _lib, ops, streaming
    from planar_optical_flow_amd.src.utils import utils
    from planar_optical_flow_amd.streaming import StreamingDetector
    text = open(os.path.join(REPO, "include", "pof_abi.h")).read()
    m = re.search(r"\bint\s+pof_grid_refine\s*\(([^)]*)\)\s*;", text)
    assert m, "include/pof_abi.h does not declare pof_grid_refine"
    params = [p.strip() for p in m.group(1).split(",")]
    restype, argtypes = _lib.SIGNATURES["pof_grid_refine"]
    assert restype is _lib._i and len(argtypes) == len(params) == 34
    for p, t in zip(params, argtypes):
        want = _lib._p if "*" in p or p.startswith("pof_stream_t") else _lib._d if p.startswith("double") else _lib._i
        assert t is want, p
    assert "N19" in text and "eps_turn" in text and "#define POF_ABI_VERSION 1" in text
    assert ops.GridRefine._fields == OUT_FIELDS
    rec = ops.grid_refine_buffers(2, device="cpu")
    assert type(rec) is ops.GridRefine and [tuple(t.shape) for t in rec] == [(2, 3), (2, 2), (2,), (2,), (2,), (2,), (2,), (2,)]
    assert [t.dtype for t in rec] == [torch.float64] * 3 + [torch.int32] * 3 + [torch.uint8] * 2
    assert not any(t.any() for t in rec)
    p = inspect.signature(ops.grid_refine).parameters
    assert list(p)[:6] == ["ranges", "tab", "rot", "trans", "pose", "state"]
    assert {k: p[k].default for k in DEFAULTS} == DEFAULTS and p["res"].kind is inspect.Parameter.KEYWORD_ONLY
    assert p["out"].default is None and "table" not in p
    assert ops.stage_settings(ops.grid_refine) == dict(DEFAULTS, res=ops.REQUIRED)
    want = {k: v for k, v in DEFAULTS.items() if k != "cls_thresh"}
    assert streaming.stage_defaults("grid_refine") == want and streaming.stage_settings("grid_refine", {}) == want
    assert streaming.stage_settings("grid_refine", dict(iters=3)) == dict(want, iters=3)
    for unknown in ("cls_thresh", "res", "size", "reach"):
        with pytest.raises(ValueError, match="unknown grid_refine settings"):
            streaming.stage_settings("grid_refine", {unknown: 1})
    assert list(inspect.signature(utils.OccupancyGrid.refine).parameters)[1:] == ["scan", "odom", "pred_cls", "pred_reg",
                                                                                  "settings"]
    assert inspect.signature(StreamingDetector.__init__).parameters["grid_refine"].default is None
    assert callable(StreamingDetector.grid_refine)
    # no CPU path
    f64 = torch.float64
    state = ops.GridMapState(torch.zeros(1, 64, 64, dtype=torch.int16), torch.zeros(1, 2, dtype=f64))
    with pytest.raises(TypeError):
        ops.grid_refine(torch.zeros(1, 4), torch.zeros(12, dtype=f64), torch.zeros(1, 2, 2), torch.zeros(1, 2, dtype=f64),
                        torch.zeros(1, 3, dtype=f64), state, res=0.1)
    with pytest.raises(TypeError):
        ops.grid_refine(None, None, None, None, None, None, res=0.1)


def test_entry_point_refuses_null_and_bad_arguments():
    import ctypes
    from planar_optical_flow_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "pof_grid_refine")
    _, argtypes = _lib.SIGNATURES["pof_grid_refine"]
    assert lib.pof_grid_refine(*[None if t is _lib._p else 0 for t in argtypes]) == _lib.POF_E_BADARG
    assert lib.pof_grid_refine(*[None if t is _lib._p else 1 for t in argtypes]) == _lib.POF_E_BADARG
    # every pointer given (never read: a refusal comes before any launch) and one bad setting at a time
    buf = ctypes.create_string_buffer(64)
    good = dict(DEFAULTS, res=0.1, B=1, N=64, H=64, W=64)

    def call(nms=(1, 1, 1), **kw):
        v = dict(good, **kw)
        ptr = ctypes.addressof(buf)
        return lib.pof_grid_refine(ptr, ptr, *[ptr if g else None for g in nms], v["cls_thresh"], v["max_range"], ptr, ptr,
                                   v["res"], v["cap"], v["iters"], v["min_points"], v["min_pivot"], v["max_shift"],
                                   v["max_turn"], v["eps_shift"], v["eps_turn"], v["B"], v["N"], v["H"], v["W"],
                                   *[ptr] * 11, None)

    nan = float("nan")
    for bad in (dict(res=0.0), dict(res=nan), dict(max_range=0.0), dict(cap=0), dict(cap=32768), dict(iters=0),
                dict(iters=33), dict(min_points=-1), dict(min_pivot=-1e-9), dict(min_pivot=nan), dict(max_shift=-1.0),
                dict(max_shift=nan), dict(max_turn=-0.01), dict(max_turn=nan), dict(B=-1), dict(N=0)):
        assert call(**bad) == _lib.POF_E_BADARG, bad
    for nms in ((1, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert call(nms=nms) == _lib.POF_E_BADARG, nms
    for bad in (dict(N=4097), dict(H=96), dict(W=32), dict(H=2112), dict(W=100)):
        assert call(**bad) == _lib.POF_E_SHAPE, bad
    assert call(B=0) == _lib.POF_OK and call(B=0, nms=(0, 0, 0)) == _lib.POF_OK
    assert call(B=0, cap=32767, iters=32, min_points=0, min_pivot=0.0, max_shift=0.0, max_turn=0.0) == _lib.POF_OK
