"""Occupancy grid map (pof_grid_map_update, N12) without a GPU: ``grid_map_oracle`` is the float64 NumPy restatement of
the comment in include/pof_abi.h, checked here rule by rule on scenes whose numbers are exact, on ray-cast rooms with
people for what the map is good for, and for the one thing a device may round differently: the beam a cell belongs to.
tests/test_grid_map_gpu.py imports the restatement and the scenes and holds the device to them bit for bit.

Rule scenes.  tests/test_person_motion.axis_table has every angle 0, so it has no beam spacing and no cell could find
its beam; ``axis_beams`` is its counterpart with angles: 9 beams, -pi + i pi / 4, whose even beams point along the axes
with exact cosines and sines (the odd ones along the diagonals carry the table's rounded values and are used as
neighbours, for a short diagonal return and for ids).  res = 0.125, the origin a multiple of res, the sensor on a cell
centre, identity and quarter-turn poses: every range, rho and border in the assertions below is a dyadic number.

Unambiguous scenes.  The only transcendental of the launch is the atan2 of the cell rule.  Every scene the GPU file
compares is built by ``device_scenes`` / ``rule_scenes`` here, and ``test_no_cell_is_near_a_beam_boundary`` asserts that
in none of them a cell with rho <= max_range has (atan2 - tab[0]) / dphi within 1e-9 of a half-integer (an atan2 that is
off by a few ulp moves the quotient by 1e-13 at most), so the device is held to equality on every cell.

Measured (this file, float64 restatement, ``people_scene(seed, 24, 0.06)`` for seeds 1-3, 256 x 256 cells of 0.1 m,
defaults): see ``test_quality_on_rooms_with_people``, which prints and DESIGN.md 8 N12 which records the figures."""
import inspect
import os
import re

import numpy as np
import pytest

from test_person_motion import IDENTITY, people_scene
from test_scan_match import add_people, angle_table, make_room, ray_cast

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = dict(cls_thresh=0.5, max_range=20.0, tol=None, hit=17, miss=8, lo=-40, hi=70, free_thresh=16)
OUT_FIELDS = ("point_cell", "point_mark", "point_prior", "det_points", "det_free")
OUT_DTYPES = (np.int32, np.uint8, np.int16, np.int32, np.int32)
QUARTER = np.array([[0.0, -1.0], [1.0, 0.0]], np.float32)
HALF_BEAM_MARGIN = 1e-9


# ---------------------------------------------------------------- restatement of the device arithmetic, one sensor
def _cell_terms(tab, rot, trans, origin, res, H, W):
    """Per cell [H,W]: rho and q = (atan2(s_y, s_x) - tab[0]) / dphi, by the header's expressions."""
    tab = np.asarray(tab, np.float64)
    N = len(tab) // 3
    Rm = np.asarray(rot, np.float32).reshape(2, 2).astype(np.float64)
    tx, ty, ox, oy = float(trans[0]), float(trans[1]), float(origin[0]), float(origin[1])
    dx = ((ox + (np.arange(W, dtype=np.float64) + 0.5) * res) - tx)[None, :]
    dy = ((oy + (np.arange(H, dtype=np.float64) + 0.5) * res) - ty)[:, None]
    sx, sy = Rm[0, 0] * dx + Rm[1, 0] * dy, Rm[0, 1] * dx + Rm[1, 1] * dy      # two products and one add each: no FMA
    rho = np.sqrt(sx * sx + sy * sy)
    dphi = tab[1] - tab[0] if N > 1 else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (np.arctan2(sy, sx) - tab[0]) / dphi
    return rho, q


def grid_map_oracle(ranges, tab, rot, trans, grid, origin, res, inst=None, num_det=None, det_cls=None, cls_thresh=0.5,
                    max_range=20.0, tol=None, hit=17, miss=8, lo=-40, hi=70, free_thresh=16):
    """One scan of one sensor.  ranges [N] float32, tab [3N], rot float32 [2,2] (or [4]), trans [2]; grid [H,W] int16 is
    UPDATED IN PLACE, origin [2]; inst [N], num_det, det_cls [N] padded like the NMS outputs, all three or none.
    -> dict of the five outputs."""
    ranges = np.asarray(ranges, np.float32)
    N, (H, W) = len(ranges), grid.shape
    tol = res if tol is None else tol
    tab = np.asarray(tab, np.float64)
    Rm = np.asarray(rot, np.float32).reshape(2, 2).astype(np.float64)
    tx, ty, ox, oy = float(trans[0]), float(trans[1]), float(origin[0]), float(origin[1])
    r = ranges.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        is_hit = np.isfinite(r) & (r > 0.0) & (r < max_range)
        px, py = r * tab[N::2], r * tab[N + 1::2]
        wx, wy = (Rm[0, 0] * px + Rm[0, 1] * py) + tx, (Rm[1, 0] * px + Rm[1, 1] * py) + ty
        gx, gy = np.floor((wx - ox) / res), np.floor((wy - oy) / res)          # a true division
        inside = is_hit & (gx >= 0.0) & (gx < W) & (gy >= 0.0) & (gy < H)      # compared in double; a NaN is outside
    at = (np.where(inside, gy, 0.0).astype(np.int64) * W + np.where(inside, gx, 0.0).astype(np.int64))
    cell = np.where(inside, at, -1).astype(np.int32)
    prior = np.where(inside, grid.reshape(-1)[at], -32768).astype(np.int16)    # before this scan's update
    det_points, det_free = np.zeros(N, np.int32), np.zeros(N, np.int32)
    person = np.zeros(N, bool)
    if inst is not None:
        nd = min(max(int(num_det), 0), N)
        inst = np.asarray(inst, np.int64)
        row_of = (inst >= 1) & (inst <= nd)
        k = np.where(row_of, inst - 1, 0)
        person = row_of & (np.asarray(det_cls, np.float64)[k] >= cls_thresh)   # pof_ego_motion's gate
        det_points[:] = np.bincount(k[inside & row_of], minlength=N)
        det_free[:] = np.bincount(k[inside & row_of & (prior.astype(np.int64) <= -free_thresh)], minlength=N)
    mark = inside & ~person
    # the cells
    rho, q = _cell_terms(tab, rot, trans, origin, res, H, W)
    with np.errstate(invalid="ignore"):
        t = np.rint(q)                                                         # to nearest, ties to even, as C's rint
        in_view = (t >= 0.0) & (t < N)                                         # a NaN and an infinity are outside
        m = np.where(in_view, t, 0.0).astype(np.int64)
        valid = ~np.isnan(r) & (r > 0.0)
    r_eff = np.where(valid, np.minimum(r, max_range), np.inf)                  # an invalid neighbour never is the minimum
    f = np.minimum(r_eff[m], np.minimum(np.where(m > 0, r_eff[np.maximum(m - 1, 0)], np.inf),
                                        np.where(m + 1 < N, r_eff[np.minimum(m + 1, N - 1)], np.inf)))
    with np.errstate(invalid="ignore"):
        freed = in_view & valid[m] & (rho + tol < f)
    burned = np.zeros(H * W, bool)
    burned[cell[mark]] = True
    burned = burned.reshape(H, W)
    delta = np.where(burned, hit, np.where(freed, -miss, 0))
    new = np.clip(grid.astype(np.int64) + delta, lo, hi).astype(np.int16)
    grid[...] = np.where(delta != 0, new, grid)                                # delta = 0 keeps the bits
    return dict(point_cell=cell, point_mark=mark.astype(np.uint8), point_prior=prior, det_points=det_points,
                det_free=det_free)


def ambiguous_cells(tab, rot, trans, origin, res, H, W, max_range):
    """How many cells with rho <= max_range have their beam quotient within HALF_BEAM_MARGIN of a half-integer."""
    rho, q = _cell_terms(tab, rot, trans, origin, res, H, W)
    with np.errstate(invalid="ignore"):
        near = np.abs(np.abs(q - np.floor(q)) - 0.5) < HALF_BEAM_MARGIN
        return int((near & (rho <= max_range) & np.isfinite(q)).sum())


def run_sensor(scene, sensor):
    """The restatement over one sensor's scans -> per scan a dict of the five outputs and ``grid`` (a copy)."""
    grid, res = np.zeros((scene["H"], scene["W"]), np.int16), []
    for s in sensor["scans"]:
        o = grid_map_oracle(s["ranges"], scene["tab"], s["rot"], s["trans"], grid, sensor["origin"], scene["res"],
                            s.get("inst"), s.get("num_det"), s.get("det_cls"), **scene["kw"])
        o["grid"] = grid.copy()
        res.append(o)
    return res


# ---------------------------------------------------------------- rule scenes: exact numbers
RES, RULE_H, RULE_W = 0.125, 64, 128
RULE_ORIGIN = np.array([-8.0, -4.0])                           # x in [-8, 8), y in [-4, 4)
CENTRE = np.array([0.0625, 0.0625])                            # the centre of cell (ix 64, iy 32)
CX, CY = 64, 32
INF, NAN = np.inf, np.nan


def axis_beams():
    """[27] table of 9 beams at -pi + i pi / 4: even beams along (-1,0), (0,-1), (1,0), (0,1), (-1,0) exactly."""
    phi = -np.pi + np.arange(9) * (np.pi / 4.0)
    cs = np.stack([np.cos(phi), np.sin(phi)], axis=1)
    cs[0::2] = [(-1.0, 0.0), (0.0, -1.0), (1.0, 0.0), (0.0, 1.0), (-1.0, 0.0)]
    return np.concatenate([phi, cs.reshape(-1)])


def _scan(ranges, rot=IDENTITY, trans=CENTRE, inst=None, num_det=None, det_cls=None):
    s = dict(ranges=np.asarray(ranges, np.float32), rot=np.asarray(rot, np.float32), trans=np.asarray(trans, np.float64))
    if inst is not None:
        cls = np.zeros(9)
        cls[:len(det_cls)] = det_cls
        s.update(inst=np.asarray(inst, np.int32), num_det=np.int32(num_det), det_cls=cls)
    return s


#            beam: 0 (-x) 1     2 (-y) 3    4 (+x)  5    6 (+y) 7    8 (-x)
BASE_RANGES = (3.0, 0.5, INF, INF, 0.9375, 2.5, 1.0, INF, 3.0)
SPOILED_RANGES = (0.0, 2.0, -1.0, 2.0, NAN, 1.0, 2.0, 2.0, 0.0)


def rule_scenes():
    """-> {name: scene}; a scene is dict(tab, H, W, res, kw, sensors=[dict(origin, scans=[...])]).  The tests below say
    what each is for."""
    kw3 = dict(DEFAULTS, max_range=3.0)
    scene = lambda kw, *scans: dict(tab=axis_beams(), H=RULE_H, W=RULE_W, res=RES, kw=kw,
                                    sensors=[dict(origin=RULE_ORIGIN, scans=list(scans))])
    gated = dict(inst=(0, 5, 0, 0, 1, -1, 2, 0, 0), num_det=2, det_cls=(0.9, 0.2))
    return {
        "base": scene(kw3, *[_scan(BASE_RANGES)] * 6),
        "quarter turn": scene(kw3, _scan(BASE_RANGES, rot=QUARTER)),
        "spoiled": scene(kw3, _scan(SPOILED_RANGES)),
        "no margin": scene(dict(kw3, tol=0.0), _scan((INF, INF, INF, INF, 1.03125, INF, INF, INF, INF))),
        "gate": scene(dict(kw3, free_thresh=8), _scan(BASE_RANGES, **gated),
                      _scan((3.0, 0.5, INF, INF, 0.5, 2.5, 1.0, INF, 3.0), **gated)),
        "clamped": scene(kw3, _scan(BASE_RANGES, inst=(0, 0, 0, 0, 9, 0, 10, 0, 0), num_det=100,
                                    det_cls=(0, 0, 0, 0, 0, 0, 0, 0, 0.9)),
                         _scan(BASE_RANGES, inst=(0, 0, 0, 0, 1, 0, 1, 0, 0), num_det=-3, det_cls=(0.9,))),
        "leaves the grid": scene(DEFAULTS, _scan((INF, INF, INF, INF, 0.9375, INF, 5.0, INF, INF))),
        "sensor outside": scene(DEFAULTS, _scan((NAN, NAN, 3.0, NAN, NAN, NAN, NAN, NAN, NAN),
                                                trans=(0.0625, 5.0625))),
    }


@pytest.fixture(scope="module")
def rules():
    scenes = rule_scenes()
    return {k: run_sensor(s, s["sensors"][0]) for k, s in scenes.items()}


def cell_of(ix, iy):
    return iy * RULE_W + ix


def test_endpoint_on_a_border_hit_priority_and_the_margin_at_equality(rules):
    o = rules["base"][0]
    g = o["grid"]
    # beam 4 (+x), r = 0.9375: w_x = 1.0, (1.0 + 8) / 0.125 = 72 exactly: the border belongs to the upper cell
    assert o["point_cell"][4] == cell_of(72, CY) and o["point_mark"][4] == 1 and o["point_prior"][4] == 0
    assert g[CY, 72] == 17                                     # a hit, although rule 2 alone would not free it either
    # rho = 0.125 k on the row of the sensor; freed while 0.125 k + 0.125 < 0.9375: k <= 6 (the sensor's own cell too)
    assert (g[CY, CX:CX + 7] == -8).all() and g[CY, 71] == 0 and (g[CY, 73:] == 0).all()
    # beam 6 (+y), r = 1.0: the endpoint in iy 40; iy 39 has rho + tol = 0.875 + 0.125 = 1.0 = f: not freed (strict <)
    assert o["point_cell"][6] == cell_of(CX, 40) and g[40, CX] == 17
    assert (g[CY:CY + 7, CX] == -8).all() and g[39, CX] == 0 and (g[41:, CX] == 0).all()
    # beam 1's endpoint, r = 0.5 on the (-,-) diagonal
    assert o["point_cell"][1] == cell_of(61, 29) and g[29, 61] == 17 and o["point_mark"][1] == 1


def test_hit_priority_over_free_in_the_same_cell(rules):
    # tol = 0 and r = 1.03125: the endpoint w_x = 1.09375 is in cell 72, whose centre has rho = 1.0 < r -- rule 2 alone
    # would free the cell, rule 1 comes first
    o = rules["no margin"][0]
    g = o["grid"]
    assert o["point_cell"][4] == cell_of(72, CY) and g[CY, 72] == 17
    assert (g[CY, CX:72] == -8).all() and (g[CY, 73:] == 0).all()


def test_three_beam_minimum_and_max_range(rules):
    o = rules["base"][0]
    g = o["grid"]
    # beam 2 (-y) has no return and would free to max_range - tol, but its neighbour 1 stops at 0.5: k <= 2 only
    assert (g[CY - 2:CY, CX] == -8).all() and (g[:CY - 2, CX] == 0).all()
    # beams 0 and 8 (-x) at r = max_range = 3.0, and inf: no hit, freed while 0.125 k + 0.125 < 3.0: k <= 22
    assert o["point_cell"][8] == -1 and o["point_prior"][8] == -32768 and o["point_mark"][8] == 0
    assert o["point_cell"][2] == -1 and o["point_mark"][2] == 0
    assert (g[CY, CX - 22:CX] == -8).all() and (g[CY, :CX - 22] == 0).all()
    assert (g == 17).sum() == 4                                # beams 1, 4, 5, 6; nothing else gained


def test_saturation_at_hi_and_lo(rules):
    hits = [int(o["grid"][CY, 72]) for o in rules["base"]]
    frees = [int(o["grid"][CY, CX + 3]) for o in rules["base"]]
    assert hits == [17, 34, 51, 68, 70, 70] and frees == [-8, -16, -24, -32, -40, -40]
    assert [int(o["point_prior"][4]) for o in rules["base"]] == [0, 17, 34, 51, 68, 70]
    last = rules["base"][-1]["grid"]
    assert last.max() == 70 and last.min() == -40


def test_quarter_turn_pose(rules):
    o = rules["quarter turn"][0]
    g = o["grid"]
    # the sensor's +x is the world's +y: beam 4 ends at w_y = 1.0, (1.0 + 4) / 0.125 = 40 exactly -> iy 40
    assert o["point_cell"][4] == cell_of(CX, 40) and g[40, CX] == 17
    assert (g[CY:CY + 7, CX] == -8).all() and g[39, CX] == 0
    # beam 6 (the sensor's +y) is the world's -x: w_x = 0.0625 - 1.0 -> ix 56; equality at ix 57
    assert o["point_cell"][6] == cell_of(56, CY) and g[CY, 56] == 17
    assert (g[CY, 58:CX + 1] == -8).all() and g[CY, 57] == 0
    assert not np.array_equal(g, rules["base"][0]["grid"]) and g.shape == (RULE_H, RULE_W)


def test_spoiled_beams_touch_nothing_and_are_no_neighbours(rules):
    o = rules["spoiled"][0]
    g = o["grid"]
    for beam in (0, 2, 4, 8):                                  # 0, negative, NaN
        assert o["point_cell"][beam] == -1 and o["point_prior"][beam] == -32768 and o["point_mark"][beam] == 0
    assert (g[CY, :] == 0).all() and (g[:CY, CX] == 0).all()   # the rows and the column of beams 8, 4 and 2: untouched
    # the (+,+) diagonal is beam 5 (r = 1.0); beam 4 is NaN and does not count: f = min(1.0, 2.0), k <= 4 freed
    diag = [int(g[CY + k, CX + k]) for k in range(1, 8)]
    assert diag == [-8, -8, -8, -8, 0, 17, 0] and o["point_cell"][5] == cell_of(70, 38)
    # the (-,-) diagonal is beam 1 (r = 2.0) between two spoiled beams: freed up to k = 10, the endpoint in k = 11
    diag = [int(g[CY - k, CX - k]) for k in range(1, 13)]
    assert diag == [-8] * 10 + [17, 0]


def test_person_gate_rows_and_counts(rules):
    first, second = rules["gate"]
    g = first["grid"]
    # beam 4 is row 0's (score 0.9): not marked, its cell neither burned in nor freed
    assert first["point_cell"][4] == cell_of(72, CY) and first["point_mark"][4] == 0 and g[CY, 72] == 0
    assert first["point_mark"][6] == 1 and g[40, CX] == 17     # row 1 is under cls_thresh: marked
    assert first["point_mark"][1] == 1 and first["point_mark"][5] == 1     # ids 5 > num_det and -1: nobody's, marked
    assert first["det_points"].tolist() == [1, 1] + [0] * 7 and not first["det_free"].any()
    # the person steps to r = 0.5: cell ix 68, freed once in the first scan (-8 <= -free_thresh = -8)
    assert second["point_cell"][4] == cell_of(68, CY) and second["point_prior"][4] == -8 and second["point_mark"][4] == 0
    assert second["det_points"].tolist() == [1, 1] + [0] * 7 and second["det_free"].tolist() == [1] + [0] * 8
    # the person's cell is not freed again (0.5 + 0.125 > 0.5) and not burned in; the cells in front of it are freed
    assert second["grid"][CY, CX:CX + 8].tolist() == [-16, -16, -16, -8, -8, -8, -8, 0] and second["point_prior"][6] == 17


def test_clamped_num_det(rules):
    first, second = rules["clamped"]
    # num_det = 100 counts as N = 9: id 9 is row 8 (score 0.9, a person), id 10 is nobody's
    assert first["point_mark"][4] == 0 and first["grid"][CY, 72] == 0 and first["point_mark"][6] == 1
    assert first["det_points"].tolist() == [0] * 8 + [1]
    # num_det = -3 counts as 0: nobody is a person, no row is written
    assert second["point_mark"][4] == 1 and second["grid"][CY, 72] == 17 and not second["det_points"].any()


def test_endpoint_outside_the_grid_and_sensor_outside_the_grid(rules):
    o = rules["leaves the grid"][0]
    assert o["point_cell"][6] == -1 and o["point_prior"][6] == -32768 and o["point_mark"][6] == 0     # w_y = 5.0625 >= 4
    assert (o["grid"][CY:, CX] == -8).all() and o["point_cell"][4] == cell_of(72, CY)
    o = rules["sensor outside"][0]
    g = o["grid"]
    # the sensor at y = 5.0625 looks down the column: the endpoint at w_y = 2.0625 is iy 48; rho + tol < 3.0 from iy 50 on
    assert o["point_cell"][2] == cell_of(CX, 48) and g[48, CX] == 17
    assert (g[50:, CX] == -8).all() and g[49, CX] == 0 and (g[:48, CX] == 0).all()
    assert (g[:, :CX - 30] == 0).all() and (g[:, CX + 30:] == 0).all()     # beam 2's wedge only: every other beam is NaN


def test_cells_without_a_change_keep_their_bits():
    scene = rule_scenes()["base"]
    grid = np.full((RULE_H, RULE_W), 99, np.int16)             # outside [lo, hi]
    s = scene["sensors"][0]["scans"][0]
    grid_map_oracle(s["ranges"], scene["tab"], s["rot"], s["trans"], grid, RULE_ORIGIN, RES, **scene["kw"])
    assert grid[0, 0] == 99 and grid[CY, 72] == 70 and grid[CY, CX] == 70 and grid[CY, 71] == 99


# ---------------------------------------------------------------- rooms
def room_scene(seed, T, N, H, W, res=0.1, sensors=1, people=True, **kw):
    """``sensors`` sensors, each in a room of its own (tests/test_scan_match.make_room / ray_cast, 1 cm noise) on a
    random walk, a 225 degree view of N beams, with tests/test_scan_match.add_people's runs of people, one of them under
    the score threshold; a few beams are inf, NaN, 0 or beyond max_range and a few ids are nobody's.  The grid is centred
    on the first pose."""
    from planar_optical_flow_amd.src.utils.utils import _pose_terms
    rng = np.random.default_rng(seed)
    tab = angle_table(N, np.radians(225.0) / N)
    out = []
    for _ in range(sensors):
        segs = make_room(rng)
        pose = np.concatenate([rng.uniform(-0.5, 0.5, 2), rng.uniform(-np.pi, np.pi, 1)])
        origin = pose[:2] - 0.5 * res * np.array([W, H])
        scans = []
        for _ in range(T):
            r = (ray_cast(segs, pose, tab[:N]) + rng.normal(0.0, 1.0, N) * 0.01).astype(np.float32)
            s = {}
            if people:
                r, inst, num, det_cls = add_people(r, rng, width=max(2, min(15, N // 8)))
                inst[rng.choice(N, 2, replace=False)] = [num + 3, -1]
                s = dict(inst=inst, num_det=np.int32(num), det_cls=det_cls)
            r[rng.choice(N, max(N // 25, 4), replace=False)] = rng.choice([np.inf, np.nan, 0.0, 25.0], max(N // 25, 4))
            rot, trans, _ = _pose_terms(pose[None])
            scans.append(dict(s, ranges=r, rot=rot[0], trans=trans[0]))
            pose = pose + np.concatenate([rng.uniform(-0.05, 0.05, 2), rng.uniform(-0.03, 0.03, 1)])
        out.append(dict(origin=origin, scans=scans))
    return dict(tab=tab, H=H, W=W, res=res, kw=dict(DEFAULTS, **kw), sensors=out)


def device_scenes():
    """-> {name: scene}: the shapes tests/test_grid_map_gpu.py runs (both forms of the points launch, one tile, H != W,
    the longest scan, the largest grid)."""
    return {
        "rooms": room_scene(31, 6, 450, 256, 256, sensors=3),
        "one tile": room_scene(32, 3, 64, 64, 64, max_range=4.0),
        "128 x 192": room_scene(33, 3, 450, 128, 192),
        "N 512": room_scene(34, 2, 512, 128, 128),
        "N 513": room_scene(35, 2, 513, 128, 128),
        "N 4096": room_scene(36, 2, 4096, 64, 128),
        "no NMS": room_scene(37, 2, 450, 128, 128, people=False),
        "2048 x 2048": room_scene(38, 1, 450, 2048, 2048, res=0.05),
    }


@pytest.mark.parametrize("which", ["rules", "device"])
def test_no_cell_is_near_a_beam_boundary(which):
    scenes = rule_scenes() if which == "rules" else device_scenes()
    cells = 0
    for name, scene in scenes.items():
        for sensor in scene["sensors"]:
            for s in sensor["scans"]:
                n = ambiguous_cells(scene["tab"], s["rot"], s["trans"], sensor["origin"], scene["res"], scene["H"],
                                    scene["W"], scene["kw"]["max_range"])
                assert n == 0, (name, n)                       # the cap is zero: re-seed a scene that breaks it
                cells += scene["H"] * scene["W"]
    print("%s scenes: %d cells looked at, none within %g of a half beam" % (which, cells, HALF_BEAM_MARGIN))


def test_device_scenes_reach_their_shapes():
    scenes = device_scenes()
    out = run_sensor(scenes["rooms"], scenes["rooms"]["sensors"][0])
    last = out[-1]
    assert (last["grid"] > 0).sum() > 100 and (last["grid"] < 0).sum() > 3000 and last["det_points"].sum() > 20
    assert last["point_mark"].sum() < (last["point_cell"] >= 0).sum()          # somebody is gated
    assert (last["point_cell"] < 0).sum() > 0 and last["det_free"].sum() > 0
    assert len(scenes["N 512"]["sensors"][0]["scans"][0]["ranges"]) == 512
    big = scenes["2048 x 2048"]
    assert (big["H"], big["W"]) == (2048, 2048) and "inst" not in scenes["no NMS"]["sensors"][0]["scans"][0]


# ---------------------------------------------------------------- what the map is good for
QUALITY_SEEDS = (1, 2, 3)


def _quality(seed, gated):
    scene = people_scene(seed, 24, 0.06)
    H = W = 256
    res = 0.1
    origin = scene["poses"][0, :2] - 0.5 * res * np.array([W, H])
    grid, outs = np.zeros((H, W), np.int16), []
    for s in scene["scans"]:
        nms = dict(inst=s["inst"], num_det=s["num_det"], det_cls=s["det_cls"]) if gated else {}
        outs.append(grid_map_oracle(s["ranges"], scene["tab"], s["rot"], s["trans"], grid, origin, res, **nms))
    # occupied cells within 0.3 m of anybody's path
    cx = origin[0] + (np.arange(W) + 0.5) * res
    cy = origin[1] + (np.arange(H) + 0.5) * res
    path = scene["truth"].reshape(-1, 2)
    d2 = ((cx[None, :, None] - path[None, None, :, 0]) ** 2 + (cy[:, None, None] - path[None, None, :, 1]) ** 2).min(axis=2)
    on_path = int(((grid > 0) & (d2 <= 0.3 ** 2)).sum())
    last, walls = outs[-1], scene["scans"][-1]["inst"] == 0
    seen = walls & (last["point_cell"] >= 0)
    res_ = dict(on_path=on_path, wall_known=float((last["point_prior"][seen] >= 17).mean()),
                wall_free=float((last["point_prior"][seen] <= -16).mean()), walkers=[], slow=[])
    if gated:
        speed = np.linalg.norm(scene["vel"], axis=1)
        for p in range(len(speed)):
            pts = sum(int(outs[t]["det_points"][scene["rows"][t, p]]) for t in range(12, 24))
            free = sum(int(outs[t]["det_free"][scene["rows"][t, p]]) for t in range(12, 24))
            if speed[p] >= 0.04:
                res_["walkers"].append(free / pts)
            elif speed[p] < 0.01:
                res_["slow"].append(free / pts)
    return res_


def test_quality_on_rooms_with_people():
    """Measured with this restatement (recorded in DESIGN.md 8, N12), seeds 1-3:
    wall points of the last scan on cells with prior >= hit: 0.998-1.000, on cells <= -free_thresh: 0 in every seed;
    occupied cells (grid > 0 after the last scan) within 0.3 m of a person's path: 0-7 with the gate, 23-34 without;
    det_free / det_points over scans 12-23: 0.69-1.00 for the four walkers (>= 0.04 m per scan), 0.01 and 0.49 for the
    two people slower than 0.01 m per scan (the second creeps 0.2 m in the sequence and leaves its old cells free)."""
    walkers, slow = [], []
    for seed in QUALITY_SEEDS:
        with_gate, without = _quality(seed, True), _quality(seed, False)
        print("seed %d: wall points known %.3f / on free cells %.3f; occupied cells on the paths %d gated, %d ungated; "
              "free share of walkers %s, of slow people %s" % (
                  seed, with_gate["wall_known"], with_gate["wall_free"], with_gate["on_path"], without["on_path"],
                  np.round(with_gate["walkers"], 2), np.round(with_gate["slow"], 2)))
        assert with_gate["on_path"] < without["on_path"]       # the gate keeps people out of the map
        assert with_gate["wall_free"] == 0.0                   # no wall point lies on a cell seen free
        # a wall point was seen before: half-way between what was measured (>= 0.998) and nothing known (0)
        assert with_gate["wall_known"] >= 0.499
        assert all(w > with_gate["wall_free"] for w in with_gate["walkers"])   # a walker's points land on free cells
        walkers += with_gate["walkers"]
        slow += with_gate["slow"]
    assert len(walkers) >= 3 and min(walkers) > max(slow + [0.0])


# ---------------------------------------------------------------- surface
def test_header_binding_and_wrappers():
    import torch
    from planar_optical_flow_amd import _lib, ops
    from planar_optical_flow_amd.src.utils import utils
    from planar_optical_flow_amd.streaming import StreamingDetector
    text = open(os.path.join(REPO, "include", "pof_abi.h")).read()
    m = re.search(r"\bint\s+pof_grid_map_update\s*\(([^)]*)\)\s*;", text)
    assert m, "include/pof_abi.h does not declare pof_grid_map_update"
    params = [p.strip() for p in m.group(1).split(",")]
    restype, argtypes = _lib.SIGNATURES["pof_grid_map_update"]
    assert restype is _lib._i and len(argtypes) == len(params) == 28
    for p, t in zip(params, argtypes):
        want = _lib._p if "*" in p or p.startswith("pof_stream_t") else _lib._d if p.startswith("double") else _lib._i
        assert t is want, p
    assert "N12" in text and "point_prior" in text
    assert ops.GridMapState._fields == ("grid", "origin") and ops.GridMapOut._fields == OUT_FIELDS
    for name in ("grid_map_update", "grid_map_buffers", "grid_map_state", "grid_map_reset"):
        assert callable(getattr(ops, name))
    p = inspect.signature(ops.grid_map_update).parameters
    assert {k: p[k].default for k in DEFAULTS} == DEFAULTS and p["res"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(p)[:5] == ["ranges", "tab", "rot", "trans", "state"]
    assert list(inspect.signature(utils.OccupancyGrid.update).parameters)[1:] == ["scan", "odom", "pred_cls", "pred_reg"]
    assert inspect.signature(StreamingDetector.__init__).parameters["grid_map"].default is None
    assert callable(StreamingDetector.grid_map)
    # no CPU path
    f64 = torch.float64
    state = ops.GridMapState(torch.zeros(1, 64, 64, dtype=torch.int16), torch.zeros(1, 2, dtype=f64))
    with pytest.raises(TypeError):
        ops.grid_map_update(torch.zeros(1, 4), torch.zeros(12, dtype=f64), torch.zeros(1, 2, 2), torch.zeros(1, 2, dtype=f64),
                            state, res=0.1)
    with pytest.raises(TypeError):
        ops.grid_map_update(None, None, None, None, None, res=0.1)
    # the wrapper refuses wrong settings before it touches a device
    for bad in (dict(size=96), dict(size=(64, 4096)), dict(res=0.0), dict(hits=3), dict(size=32)):
        with pytest.raises(ValueError):
            utils.OccupancyGrid(np.zeros(4), **bad)


def test_entry_point_refuses_null_and_bad_arguments():
    import ctypes
    from planar_optical_flow_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "pof_grid_map_update")
    _, argtypes = _lib.SIGNATURES["pof_grid_map_update"]
    assert lib.pof_grid_map_update(*[None if t is _lib._p else 0 for t in argtypes]) == _lib.POF_E_BADARG
    assert lib.pof_grid_map_update(*[None if t is _lib._p else 1 for t in argtypes]) == _lib.POF_E_BADARG
