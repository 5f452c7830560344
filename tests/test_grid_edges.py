"""The occupancy-grid stages (pof_grid_map_update N12, pof_grid_match N13) where tiles, slices and limits decide: the
scene builders of tests/test_grid_edges_gpu.py and, without a GPU, the conditions those scenes have to meet.  The
referees are the restatements of tests/test_grid_map.py and tests/test_grid_match.py, unchanged; what is new is the
inputs.

A. Map.  Every sensor starts from a PRIOR grid that is not empty (``prior_grid``: values inside [lo, hi], at lo, at hi and
a few outside), so a tile that is wrongly skipped and a tile that is wrongly rewritten both show.  ``tile_exits`` restates
the two early exits of grid_cells_kernel in float64 without FMA; it is no referee, it only says where a scene stands:
  * ``free_edge_scenes``: dyadic scenes (res 0.125, the sensor on a cell centre inside the grid, outside each of its four
    sides and beyond a corner, identity and quarter turn, no beam with a return) whose max_range puts the nearest cell of
    a named tile at rho + tol == max_range exactly -- the exit fires and the restatement frees nothing there -- and the
    same scene at nextafter(max_range), where the tile is kept and the restatement frees its nearest cell;
  * ``hit_edge_scenes``: single returns in the first and the last column and row of a named tile and in the first cell
    beyond it, at rotation 0 (axis beams, the box of reachable cells ends exactly on that column or row) and at 45
    degrees (the float32 terms of ``_pose_terms``, 450 beams, the box at its loosest);
  * ``general_scenes``: 24 ray-cast rooms, the sensor anywhere in a box 1.5 times the grid at any rotation, max_range
    around one and two tile widths, on 256 x 256 and 64 x 256 cells of 0.05 m at four coordinate magnitudes (origin near
    0, 2^20, -2^30 and 2^36 m);
  * ``small_table_scenes`` (N = 1, 2, 3) and ``spoiled_pose_scenes`` (NaN, +inf, -inf in rot, trans or origin beside a
    healthy sensor).

B. Match.  ``match_cases``: every reach from 0 to 16 (every slice count of grid_match_scores_kernel), long scans with
a wide search, grids of 2048 cells a side with staged points on all four borders (the packed LDS cell), scores at
+-4096 x 32767 with the gates at 0, 32767 and 2^31 - 1, all-equal and all-tied candidates at the largest search, the four
coordinate magnitudes, N = 1 and non-finite pose terms.  Every case is also held to ``literal_scores``; where the literal
triple loop would take seconds (it is written for the rule scenes) the scan is thinned for that check -- the ranges of all
but every s-th voting point set to NaN -- and the restatement and the loop are compared on the thinned scan, s = 1 (the
whole case) wherever the loop stays under LITERAL_BUDGET steps.

Measured without a GPU (``pytest tests/test_grid_edges.py --durations=0``, each run alone on the same machine): this file
6.9 s, of which about 2.4 s are the first import of torch (charged to the hit-edge test, 1.7-2.4 s), 2.3 s the match
cases with their restatement (the fixture), 2.3 s the literal loops, 0.2 s each the can_free and the general family;
tests/test_grid_map.py + tests/test_grid_match.py together 8.4 s, the same import included."""
import copy

import numpy as np
import pytest

from test_grid_map import (DEFAULTS as MAP_DEFAULTS, INF, NAN, QUARTER, ambiguous_cells, axis_beams, grid_map_oracle,
                           room_scene)
from test_grid_match import (BASE_RANGES, DEFAULTS as MATCH_DEFAULTS, RES as RULE_RES, RULE_H, RULE_W, _sensor,
                             literal_scores, noise_grid, painted, pose_terms, room_case,
                             rotation_table, run_case, voting_points)
from test_person_motion import IDENTITY
from test_scan_match import angle_table, make_room, ray_cast

TILE = 64
MAGNITUDES = (0.0, 2.0 ** 20, -2.0 ** 30, 2.0 ** 36)
NON_FINITE = (("NaN", NAN), ("+inf", INF), ("-inf", -INF))


# ================================================================ A. the map
def prior_grid(seed, H, W, lo=MAP_DEFAULTS["lo"], hi=MAP_DEFAULTS["hi"]):
    """A grid that is not empty: 78 % anywhere in [lo, hi], 10 % at lo, 10 % at hi, 1.5 % outside (99 and -99, the trick
    of tests/test_grid_map.test_cells_without_a_change_keep_their_bits: only a cell that is written is clamped)."""
    rng = np.random.default_rng(seed)
    g, u = rng.integers(lo, hi + 1, (H, W)).astype(np.int16), rng.random((H, W))
    g[u < 0.10], g[u > 0.90] = lo, hi
    g[(u > 0.495) & (u < 0.505)], g[(u > 0.595) & (u < 0.600)] = 99, -99
    return g


def map_scene(tab, H, W, res, sensors, **kw):
    return dict(tab=np.asarray(tab, np.float64), H=H, W=W, res=res, kw=dict(MAP_DEFAULTS, **kw), sensors=list(sensors))


def map_sensor(origin, prior, ranges, rot, trans, **nms):
    scan = dict(nms, ranges=np.asarray(ranges, np.float32), rot=np.asarray(rot, np.float32).reshape(2, 2).copy(),
                trans=np.asarray(trans, np.float64).copy())
    return dict(origin=np.asarray(origin, np.float64).copy(), prior=prior, scans=[scan])


def run_prior(scene, sensor):
    """tests/test_grid_map.run_sensor from the sensor's prior grid: per scan the five outputs and ``grid`` (a copy)."""
    grid, res = sensor["prior"].copy(), []
    for s in sensor["scans"]:
        o = grid_map_oracle(s["ranges"], scene["tab"], s["rot"], s["trans"], grid, sensor["origin"], scene["res"],
                            s.get("inst"), s.get("num_det"), s.get("det_cls"), **scene["kw"])
        o["grid"] = grid.copy()
        res.append(o)
    return res


def deltas(scene, sensor):
    """What the restatement does to every cell with the sensor's one scan, [H,W]: +1 burned in, -1 freed, 0 nothing --
    read from a run on an empty grid (which cells change does not depend on what they hold)."""
    empty = dict(sensor, prior=np.zeros((scene["H"], scene["W"]), np.int16))
    return np.sign(run_prior(scene, empty)[0]["grid"]).astype(np.int64)


def tile_kinds(delta):
    """[H/64, W/64]: 0 an untouched tile, 1 one with burned-in cells, 2 one with freed cells and none burned in."""
    H, W = delta.shape
    t = delta.reshape(H // TILE, TILE, W // TILE, TILE)
    burned, freed = (t > 0).any(axis=(1, 3)), (t < 0).any(axis=(1, 3))
    return np.where(burned, 1, np.where(freed, 2, 0))


def _bound(vals):
    vals = np.asarray(vals, np.float64)
    if (vals > 0.0).all():
        return vals.min()
    if (vals < 0.0).all():
        return -vals.max()
    return np.float64(0.0)


def tile_exits(scene, scan, origin, x0, y0):
    """Where a scene stands against the two early exits of grid_cells_kernel for the tile at cell (x0, y0), in the
    kernel's own expressions (float64, products and sums rounded one by one) -> (rho_lb, can_free, can_hit)."""
    f = np.float64
    r00, r01, r10, r11 = np.asarray(scan["rot"], np.float32).reshape(4).astype(np.float64)
    tx, ty, ox, oy = f(scan["trans"][0]), f(scan["trans"][1]), f(origin[0]), f(origin[1])
    res, mr = f(scene["res"]), f(scene["kw"]["max_range"])
    tol = res if scene["kw"]["tol"] is None else f(scene["kw"]["tol"])
    last = TILE - 1
    with np.errstate(all="ignore"):
        dxa, dxb = (ox + (f(x0) + 0.5) * res) - tx, (ox + (f(x0 + last) + 0.5) * res) - tx
        dya, dyb = (oy + (f(y0) + 0.5) * res) - ty, (oy + (f(y0 + last) + 0.5) * res) - ty
        lbx = _bound([r00 * dxa + r10 * dya, r00 * dxa + r10 * dyb, r00 * dxb + r10 * dya, r00 * dxb + r10 * dyb])
        lby = _bound([r01 * dxa + r11 * dya, r01 * dxa + r11 * dyb, r01 * dxb + r11 * dya, r01 * dxb + r11 * dyb])
        rho_lb = np.sqrt(lbx * lbx + lby * lby)
        can_free = not (rho_lb + tol >= mr)
        ex, ey = np.abs(r00) * mr + np.abs(r01) * mr, np.abs(r10) * mr + np.abs(r11) * mr
        gxa, gxb = np.floor(((tx - ex) - ox) / res), np.floor(((tx + ex) - ox) / res)
        gya, gyb = np.floor(((ty - ey) - oy) / res), np.floor(((ty + ey) - oy) / res)
        can_hit = not (gxb < x0 or gxa > x0 + last or gyb < y0 or gya > y0 + last)
    return rho_lb, can_free, can_hit


def exits_are_sound(scene, sensor, delta):
    """No tile that an exit would skip holds a cell the restatement changes -> (tiles without frees, without hits)."""
    no_free = no_hit = 0
    for ty in range(scene["H"] // TILE):
        for tx in range(scene["W"] // TILE):
            _, can_free, can_hit = tile_exits(scene, sensor["scans"][0], sensor["origin"], tx * TILE, ty * TILE)
            d = delta[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE]
            assert can_free or not (d < 0).any(), (tx, ty, "freed cells in a tile the exit skips")
            assert can_hit or not (d > 0).any(), (tx, ty, "burned cells in a tile the exit skips")
            no_free, no_hit = no_free + (not can_free), no_hit + (not can_hit)
    return no_free, no_hit


def no_ambiguous_cell(scene):
    for sensor in scene["sensors"]:
        for s in sensor["scans"]:
            n = ambiguous_cells(scene["tab"], s["rot"], s["trans"], sensor["origin"], scene["res"], scene["H"],
                                scene["W"], scene["kw"]["max_range"])
            assert n == 0, n                                   # the cap is zero: re-seed a scene that breaks it


# ---------------------------------------------------------------- exact boundary of can_free
E_RES = 0.125
E_ORIGIN = {(256, 256): (-16.0, -16.0), (64, 256): (-16.0, -4.0)}
# name: (H, W), the sensor's cell (ix, iy) -- outside the grid where an index is -- , rot, the named tile (tx, ty), and
# the whole cells (kx, ky) between the sensor and the tile's nearest cell centre: rho = hypot(kx, ky) res, exact
FREE_EDGES = {
    "inside, along x": ((256, 256), (40, 70), IDENTITY, (1, 1), (24, 0)),
    "inside, along x, quarter turn": ((256, 256), (40, 70), QUARTER, (1, 1), (24, 0)),
    "inside, 6-8-10": ((256, 256), (58, 56), IDENTITY, (1, 1), (6, 8)),
    "inside, 6-8-10, quarter turn": ((256, 256), (58, 56), QUARTER, (1, 1), (6, 8)),
    "inside, from above and the right": ((256, 256), (139, 136), IDENTITY, (1, 1), (12, 9)),
    "left of the grid": ((64, 256), (-9, 30), IDENTITY, (0, 0), (9, 0)),
    "right of the grid": ((64, 256), (264, 30), QUARTER, (3, 0), (9, 0)),
    "below the grid": ((64, 256), (100, -9), QUARTER, (1, 0), (0, 9)),
    "above the grid": ((64, 256), (100, 72), IDENTITY, (1, 0), (0, 9)),
    "beyond the corner": ((256, 256), (-3, -4), IDENTITY, (0, 0), (3, 4)),
    "beyond the far corner, quarter turn": ((256, 256), (261, 263), QUARTER, (3, 3), (6, 8)),
}


def free_edge_scenes():
    """-> {(name, "at" | "above"): scene}, one sensor each, every beam without a return (f = max_range everywhere)."""
    out = {}
    for seed, (name, ((H, W), (ix, iy), rot, _, (kx, ky))) in enumerate(FREE_EDGES.items()):
        origin = np.array(E_ORIGIN[(H, W)])
        trans = origin + (np.array([ix, iy]) + 0.5) * E_RES
        at = float(np.hypot(kx, ky)) * E_RES + E_RES           # rho + tol of the nearest cell, a dyadic number
        for which, max_range in (("at", at), ("above", float(np.nextafter(at, np.inf)))):
            sensor = map_sensor(origin, prior_grid(100 + seed, H, W), [INF] * 9, rot, trans)
            out[(name, which)] = map_scene(axis_beams(), H, W, E_RES, [sensor], max_range=max_range)
    return out


def test_free_edge_scenes_stand_on_the_boundary():
    scenes, freed_above = free_edge_scenes(), 0
    for (name, which), scene in scenes.items():
        (H, W), _, _, (tx, ty), (kx, ky) = FREE_EDGES[name]
        sensor = scene["sensors"][0]
        no_ambiguous_cell(scene)
        delta = deltas(scene, sensor)
        exits_are_sound(scene, sensor, delta)
        rho_lb, can_free, _ = tile_exits(scene, sensor["scans"][0], sensor["origin"], tx * TILE, ty * TILE)
        tile = delta[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE]
        assert rho_lb == np.hypot(kx, ky) * E_RES and not (delta > 0).any(), (name, which)
        if which == "at":
            assert rho_lb + E_RES == scene["kw"]["max_range"] and not can_free, name      # equality: the exit fires
            assert not tile.any(), name                                                   # and nothing is freed
        else:
            assert can_free and (tile < 0).sum() >= 1, name                               # one ulp more: kept, and freed
            freed_above += int((tile < 0).sum())
        want = run_prior(scene, sensor)[0]["grid"]
        kept = tile == 0
        assert np.array_equal(want[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE][kept],
                              sensor["prior"][ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE][kept])
    outside = sum(1 for (H, W), (ix, iy), *_ in FREE_EDGES.values() if not (0 <= ix < W and 0 <= iy < H))
    print("can_free boundary: %d scenes (%d with the sensor outside the grid), the named tile exits at equality in every "
          "one and has %d freed cells in all one ulp above" % (len(scenes), 2 * outside, freed_above))
    assert outside >= 5


# ---------------------------------------------------------------- exact boundary of can_hit
H_TILE = (1, 1)                                                # the named tile: cells 64..127 both ways


def hit_edge_axis(shift, rot=IDENTITY):
    """Four sensors around the named tile of a 256 x 256 grid, each with one return (r = 23.625 cells, max_range = 23.75
    cells) straight into the tile's first column, last column, first row, last row (shift 0; the box of reachable cells
    ends exactly there) or, one cell further away, into the first cell in front of the tile (shift 1: the tile exits).
    -> (scene, the four cells (ix, iy))."""
    origin = np.array(E_ORIGIN[(256, 256)])
    r, max_range = 23.625 * E_RES, 23.75 * E_RES
    turned = np.array_equal(rot, QUARTER)
    # sensor cell, the beam that looks at the tile (axis_beams: 0/8 -x, 2 -y, 4 +x, 6 +y; a quarter turn maps the
    # sensor's +x to the world's +y), the cell of the endpoint
    rows = (((40 - shift, 70), 2 if turned else 4, (64 - shift, 70)), ((151 + shift, 70), 6 if turned else 8, (127 + shift, 70)),
            ((70, 40 - shift), 4 if turned else 6, (70, 64 - shift)), ((70, 151 + shift), 8 if turned else 2, (70, 127 + shift)))
    sensors, cells = [], []
    for k, (at, beam, cell) in enumerate(rows):
        ranges = [INF] * 9
        ranges[beam] = r
        if beam == 8:
            ranges[0] = r                                      # the same direction
        sensors.append(map_sensor(origin, prior_grid(200 + 10 * shift + k, 256, 256), ranges, rot,
                                  origin + (np.array(at) + 0.5) * E_RES))
        cells.append(cell)
    return map_scene(axis_beams(), 256, 256, E_RES, sensors, max_range=max_range), cells


# the diagonal scene: (axis, the column or row of cells, the cell index across it to aim at)
DIAGONAL_TARGETS = (("x", 64, 80), ("x", 64, 120), ("x", 127, 70), ("x", 127, 110), ("y", 64, 75), ("y", 64, 115),
                    ("y", 127, 72), ("y", 127, 110), ("x", 128, 75), ("x", 128, 100), ("y", 128, 80), ("y", 128, 105),
                    ("x", 63, 85), ("y", 63, 85))
DIAGONAL_AT = (30.37, 28.61)                                   # the sensor in cells from the origin: on no cell centre


def hit_edge_diagonal():
    """One sensor at 45 degrees (rot: what ``_pose_terms`` writes in float32) with 14 single returns, each on the centre
    line of a column or row: the first and last column and row of the named tile and the first cells beyond it.
    -> (scene, the cells (ix, iy) of the returns, computed here in plain float64)."""
    from planar_optical_flow_amd.src.utils.utils import _pose_terms
    N = 450
    tab = angle_table(N, np.radians(225.0) / N)
    origin = np.array(E_ORIGIN[(256, 256)])
    pose = np.concatenate([origin + np.array(DIAGONAL_AT) * E_RES, [np.pi / 4]])
    rot, trans, _ = _pose_terms(pose[None])
    Rm = rot[0].astype(np.float64)
    d = np.stack([Rm[0, 0] * tab[N::2] + Rm[0, 1] * tab[N + 1::2], Rm[1, 0] * tab[N::2] + Rm[1, 1] * tab[N + 1::2]], axis=1)
    ranges, cells = np.full(N, INF, np.float32), []
    for axis, line, across in DIAGONAL_TARGETS:
        a = 0 if axis == "x" else 1
        want = origin + (np.array([line, across] if a == 0 else [across, line]) + 0.5) * E_RES - trans[0]
        beam = int(np.argmax(d @ (want / np.linalg.norm(want))))
        assert ranges[beam] == INF                             # one return per beam
        ranges[beam] = np.float32(want[a] / d[beam, a])        # onto the centre line of the column (row)
        w = trans[0] + np.float64(ranges[beam]) * d[beam]
        cells.append(tuple(int(v) for v in np.floor((w - origin) / E_RES)))
    finite = ranges[np.isfinite(ranges)]
    sensor = map_sensor(origin, prior_grid(230, 256, 256), ranges, rot[0], trans[0])
    return map_scene(tab, 256, 256, E_RES, [sensor], max_range=float(finite.max()) + 0.25), cells


def hit_edge_scenes():
    """-> {name: (scene, per sensor the cells its returns are aimed at)}."""
    out = {}
    for shift, what in ((0, "edge of the tile"), (1, "first cell beyond")):
        for rot, turn in ((IDENTITY, "rotation 0"), (QUARTER, "quarter turn")):
            scene, cells = hit_edge_axis(shift, rot)
            out["%s, %s" % (what, turn)] = (scene, [[c] for c in cells])
    scene, cells = hit_edge_diagonal()
    out["45 degrees"] = (scene, [cells])
    return out


def test_hit_edge_scenes_burn_exactly_the_aimed_cells():
    x0, y0 = H_TILE[0] * TILE, H_TILE[1] * TILE
    for name, (scene, aimed) in hit_edge_scenes().items():
        no_ambiguous_cell(scene)
        in_tile = beyond = 0
        for sensor, cells in zip(scene["sensors"], aimed):
            delta = deltas(scene, sensor)
            exits_are_sound(scene, sensor, delta)
            burned = {(int(x), int(y)) for y, x in zip(*np.nonzero(delta > 0))}
            assert burned == set(cells) and len(set(cells)) == len(cells), (name, burned, cells)
            _, can_free, can_hit = tile_exits(scene, sensor["scans"][0], sensor["origin"], x0, y0)
            inside = [c for c in cells if x0 <= c[0] < x0 + TILE and y0 <= c[1] < y0 + TILE]
            assert can_hit == bool(inside) or name == "45 degrees", (name, can_hit)       # the box ends on the cell
            in_tile, beyond = in_tile + len(inside), beyond + len(cells) - len(inside)
            # a burned cell takes +hit from its prior, clamped; nothing else of the grid gains
            want = run_prior(scene, sensor)[0]["grid"].astype(np.int64)
            for x, y in cells:
                assert want[y, x] == min(max(int(sensor["prior"][y, x]) + 17, -40), 70)
        if name == "45 degrees":
            cells = aimed[0]
            edges = [sum(1 for c in cells if c[a] == v and x0 <= c[1 - a] < x0 + TILE) for a in (0, 1) for v in (64, 127)]
            past = [sum(1 for c in cells if c[a] == v) for a in (0, 1) for v in (63, 128)]
            assert min(edges) >= 2 and min(past) >= 1, (edges, past)
            rot = scene["sensors"][0]["scans"][0]["rot"]
            assert rot.dtype == np.float32 and abs(abs(rot[0, 0]) - abs(rot[0, 1])) < 1e-7    # the box at its loosest
        print("can_hit boundary, %s: %d returns in the named tile, %d beyond it, burned in exactly there"
              % (name, in_tile, beyond))
        assert (in_tile > 0) == (not name.startswith("first cell beyond")) and (beyond > 0) == (not name.startswith("edge"))


# ---------------------------------------------------------------- general position
G_RES, G_N = 0.05, 450
G_RANGES = (1.6, 3.2, float(np.nextafter(3.2, np.inf)), 4.75, 6.4, 9.0)          # a tile is 3.2 m wide
G_SCENES = 24
G_SEEDS = {}                                                   # scene index -> another seed, for a broken condition


def general_scene(i):
    """Scene i of the family: -> (scene, magnitude index, small grid).  One sensor in a ray-cast room of its own (1 cm
    noise, a few beams inf, NaN, 0 or far), anywhere in a box 1.5 times the grid around the grid's middle, any rotation."""
    from planar_optical_flow_amd.src.utils.utils import _pose_terms
    rng = np.random.default_rng(G_SEEDS.get(i, 700 + i))
    small = i % 3 == 2
    H, W = (64, 256) if small else (256, 256)
    M = MAGNITUDES[i % 4]
    tab = angle_table(G_N, np.radians(225.0) / G_N)
    origin = np.array([M, M]) + rng.uniform(-1.0, 1.0, 2)
    at = origin + (0.5 + 1.5 * (rng.uniform(0.0, 1.0, 2) - 0.5)) * np.array([W, H]) * G_RES
    phi = rng.uniform(-np.pi, np.pi)
    local = np.concatenate([rng.uniform(-0.5, 0.5, 2), [phi]])                   # the sensor in its room
    r = (ray_cast(make_room(rng), local, tab[:G_N]) + rng.normal(0.0, 1.0, G_N) * 0.01).astype(np.float32)
    r[rng.choice(G_N, 18, replace=False)] = rng.choice([np.inf, np.nan, 0.0, 25.0], 18)
    rot, trans, _ = _pose_terms(np.concatenate([at, [phi]])[None])
    sensor = map_sensor(origin, prior_grid(800 + i, H, W), r, rot[0], trans[0])
    return map_scene(tab, H, W, G_RES, [sensor], max_range=G_RANGES[(i // 4) % 6]), i % 4, small


def general_scenes():
    return [general_scene(i) for i in range(G_SCENES)]


def _touching(kinds):
    """An untouched tile shares an edge with a touched one."""
    u = kinds == 0
    return bool((u[1:] & ~u[:-1]).any() or (u[:-1] & ~u[1:]).any() or (u[:, 1:] & ~u[:, :-1]).any()
                or (u[:, :-1] & ~u[:, 1:]).any())


def test_general_family_meets_its_conditions():
    total, by_mag, by_small = np.zeros(3, int), np.zeros((4, 3), int), np.zeros(3, int)
    touching = outside = skipped_free = skipped_hit = 0
    for i, (scene, mag, small) in enumerate(general_scenes()):
        sensor = scene["sensors"][0]
        no_ambiguous_cell(scene)
        delta = deltas(scene, sensor)
        no_free, no_hit = exits_are_sound(scene, sensor, delta)
        skipped_free, skipped_hit = skipped_free + no_free, skipped_hit + no_hit
        kinds = tile_kinds(delta)
        counts = np.bincount(kinds.ravel(), minlength=3)
        total += counts
        by_mag[mag] += counts
        by_small += counts * small
        touching += _touching(kinds)
        cell = (sensor["scans"][0]["trans"] - sensor["origin"]) / G_RES
        outside += not (0 <= cell[0] < scene["W"] and 0 <= cell[1] < scene["H"])
        want = run_prior(scene, sensor)[0]["grid"]
        assert np.array_equal(want[delta == 0], sensor["prior"][delta == 0])    # what is not touched keeps its bits
    print("general position: %d scenes, %d with the sensor outside its grid; tiles untouched / burned in / freed only: "
          "%s in all, %s on 64 x 256, per magnitude %s; an untouched tile beside a touched one in %d scenes; tiles "
          "whose exit skips the frees %d, the hits %d" % (G_SCENES, outside, total.tolist(), by_small.tolist(),
                                                          by_mag.tolist(), touching, skipped_free, skipped_hit))
    assert G_SCENES >= 24 and (total >= 20).all(), total
    assert 2 * touching >= G_SCENES, touching
    assert (by_small >= 1).all() and (by_mag >= 1).all(), (by_small, by_mag)
    assert outside >= 3 and skipped_free >= 20 and skipped_hit >= 20


# ---------------------------------------------------------------- smallest tables, non-finite pose terms
def small_table_scenes():
    """N = 1 (dphi = 0: no cell finds a beam, the point still burns in), 2 and 3 on one tile."""
    origin, pose = np.array([-4.0, -4.0]), np.array([0.07, -0.11, 0.4])
    rot, trans = pose_terms(pose)
    out = {}
    for N, ranges in ((1, [1.5]), (2, [1.5, INF]), (3, [2.0, 0.75, INF])):
        sensor = map_sensor(origin, prior_grid(300 + N, 64, 64), ranges, rot, trans)
        out["N %d" % N] = map_scene(angle_table(N, np.radians(50.0)), 64, 64, E_RES, [sensor], max_range=3.0)
    return out


def spoiled_pose_scenes():
    """-> {(field, value name): scene of two sensors}: sensor 0 has one element of rot, trans or origin spoiled, sensor 1
    is healthy; rooms with people as tests/test_grid_map.room_scene builds them."""
    out = {}
    for f, field in enumerate(("rot", "trans", "origin")):
        for v, (name, value) in enumerate(NON_FINITE):
            base = room_scene(310 + 3 * f + v, 1, 450, 128, 128, sensors=2, max_range=6.0)
            for b, sensor in enumerate(base["sensors"]):
                sensor["prior"] = prior_grid(320 + 10 * f + 2 * v + b, 128, 128)
                sensor["origin"] = np.asarray(sensor["origin"], np.float64).copy()
                sensor["scans"][0]["rot"] = sensor["scans"][0]["rot"].copy()
                sensor["scans"][0]["trans"] = sensor["scans"][0]["trans"].copy()
            spoiled = base["sensors"][0]
            where = spoiled if field == "origin" else spoiled["scans"][0]
            where[field].reshape(-1)[(f + v) % where[field].size] = value
            out[(field, name)] = base
    return out


def test_small_tables_and_spoiled_pose_terms():
    for name, scene in small_table_scenes().items():
        no_ambiguous_cell(scene)
        sensor = scene["sensors"][0]
        delta = deltas(scene, sensor)
        exits_are_sound(scene, sensor, delta)
        assert (delta > 0).sum() == {"N 1": 1, "N 2": 1, "N 3": 2}[name]
        assert ((delta < 0).sum() == 0) == (name == "N 1"), name               # dphi = 0 lands outside
        print("%s: %d cells burned in, %d freed" % (name, (delta > 0).sum(), (delta < 0).sum()))
    for (field, value), scene in spoiled_pose_scenes().items():
        no_ambiguous_cell(scene)
        spoiled, healthy = scene["sensors"]
        o = run_prior(scene, spoiled)[0]
        assert np.array_equal(o["grid"], spoiled["prior"]), (field, value)     # the spoiled sensor's grid is unchanged
        assert (o["point_cell"] == -1).all() and not o["point_mark"].any() and not o["det_points"].any()
        h = run_prior(scene, healthy)[0]
        assert (h["grid"] != healthy["prior"]).sum() > 1000 and h["det_points"].sum() > 0, (field, value)
    print("non-finite pose terms: %d scenes, the spoiled sensor's grid unchanged in every one" % len(spoiled_pose_scenes()))


# ================================================================ B. the match
LITERAL_BUDGET = 30000                                         # steps of the literal triple loop per sensor


def with_search(case, **kw):
    return dict(case, kw=dict(case["kw"], **kw))


def reach_cases():
    """Every reach from 0 to 16 at 1 and 3 rotations, and 33 rotations at reach 5 and 16: N = 450 on 64 x 128 cells; one
    room, its last scan 0.2 m and 0.012 rad off.  S = max(1, 256 / (T T)) = 256, 28, 10, 5, 3, 2, 1, ... slices."""
    base = room_case(81, 450, 64, 128, scans=4, offsets=((0.17, -0.12, 0.012),), min_points=20, min_score=5, min_gain=2)
    out = {"reach %d, %d rotations" % (R, K): with_search(base, reach=R, rotations=K) for R in range(17) for K in (1, 3)}
    out.update({"reach %d, 33 rotations" % R: with_search(base, reach=R, rotations=33, rot_step=0.002) for R in (5, 16)})
    return out


def long_scan_cases():
    # most of a room's points end outside 6.4 m x 12.8 m of grid, and a voting point outside adds nothing: low gates
    gates = dict(min_points=20, min_score=2, min_gain=2)
    long = room_case(82, 4096, 64, 128, scans=3, offsets=((0.23, -0.17, 0.021),), reach=8, rotations=3, **gates)
    return {"N 4096, reach 8": long, "N 4096, reach 16": with_search(long, reach=16),
            "N 513, reach 16": room_case(83, 513, 128, 128, scans=3, offsets=((-0.31, 0.12, -0.03),), reach=16, rotations=3,
                                         **gates)}


PACK_REACH, PACK_N, PACK_RES = 16, 1024, 0.05
PACK_SHAPES = ((2048, 2048), (64, 2048), (2048, 64))


def packing_case(H, W, seed):
    """A sensor in the middle of an H x W grid whose 1024 beams, all around, end on a rectangle that lies -24 to +24
    cells from the grid's border, beam by beam: staged cells on both sides of all four borders, and cells beyond reach.
    The grid is painted in bands of 48 cells along its borders."""
    rng = np.random.default_rng(seed)
    tab = angle_table(PACK_N, 2.0 * np.pi / PACK_N)
    pose = np.array([0.013, -0.021, 0.1])
    rot, trans = pose_terms(pose)
    origin = -0.5 * PACK_RES * np.array([W, H], np.float64)
    ang = tab[:PACK_N] + pose[2]
    off = rng.integers(-24, 25, (PACK_N, 2)) + 0.5
    half = (0.5 * np.array([W, H]) + off) * PACK_RES
    r = np.minimum(half[:, 0] / np.abs(np.cos(ang)), half[:, 1] / np.abs(np.sin(ang))).astype(np.float32)
    grid = np.zeros((H, W), np.int16)
    band = rng.integers(-40, 71, (H, W)).astype(np.int16)
    for sl in (np.s_[:48], np.s_[-48:], np.s_[:, :48], np.s_[:, -48:]):
        grid[sl] = band[sl]
    sensor = dict(ranges=r, rot=rot.reshape(2, 2), trans=trans, pose=pose, grid=grid, origin=origin)
    kw = dict(MATCH_DEFAULTS, max_range=200.0, reach=PACK_REACH, rotations=3, min_points=10, min_score=1, min_gain=1)
    return dict(tab=tab, H=H, W=W, res=PACK_RES, kw=kw, sensors=[sensor])


def packing_cases():
    return {"%d x %d" % (H, W): packing_case(H, W, 90 + k) for k, (H, W) in enumerate(PACK_SHAPES)}


def border_bands(cells, H, W, R):
    """How many cells [n,2] = (g_x, g_y) lie within R outside each border: (left, right, below, above)."""
    gx, gy = cells[:, 0], cells[:, 1]
    near_y, near_x = (gy >= -R) & (gy < H + R), (gx >= -R) & (gx < W + R)
    return (int(((gx >= -R) & (gx < 0) & near_y).sum()), int(((gx >= W) & (gx < W + R) & near_y).sum()),
            int(((gy >= -R) & (gy < 0) & near_x).sum()), int(((gy >= H) & (gy < H + R) & near_x).sum()))


X_N = 4096
GATES = (0, 32767, 2 ** 31 - 1)


def parity_sensor(H, W, r0, grid, res=0.1):
    """4096 beams all around, every one with a return inside the H x W grid on a cell whose ix + iy is even, at least a
    thousandth of a cell from the cell's borders; the first such range from r0 on in steps of a sixteenth of a cell."""
    tab = angle_table(X_N, 2.0 * np.pi / X_N)
    pose = np.array([0.03, -0.02, 0.2])
    rot, trans = pose_terms(pose)
    origin = -0.5 * res * np.array([W, H], np.float64)
    Rm = rot.reshape(2, 2).astype(np.float64)
    d = np.stack([Rm[0, 0] * tab[X_N::2] + Rm[0, 1] * tab[X_N + 1::2], Rm[1, 0] * tab[X_N::2] + Rm[1, 1] * tab[X_N + 1::2]], axis=1)
    r = (r0 + 0.0625 * res * np.arange(240)).astype(np.float32).astype(np.float64)
    g = (trans[None, None] + r[None, :, None] * d[:, None] - origin) / res                # [N, 240, 2]
    frac = g - np.floor(g)
    good = ((np.floor(g).sum(axis=2) % 2 == 0) & (frac > 0.001).all(axis=2) & (frac < 0.999).all(axis=2)
            & (g >= 0).all(axis=2) & (g[..., 0] < W) & (g[..., 1] < H))
    assert good.any(axis=1).all()
    ranges = r[np.argmax(good, axis=1)].astype(np.float32)
    return tab, dict(ranges=ranges, rot=rot.reshape(2, 2), trans=trans, pose=pose, grid=grid, origin=origin)


def extreme_cases():
    """-> {name: case}: grids all 32767, all -32768 and a +-32767 checkerboard (-32767 where ix + iy is even, where every
    point stands) under 4096 voting points, each with min_score = min_gain = 0, 32767 and 2^31 - 1; and the all -32768
    grid of one tile with the points close to its border, where shifting points out of the grid is what scores best."""
    yy, xx = np.mgrid[:128, :128]
    grids = {"all 32767": np.full((128, 128), 32767, np.int16), "all -32768": np.full((128, 128), -32768, np.int16),
             "checkerboard": np.where((xx + yy) % 2 == 0, -32767, 32767).astype(np.int16)}
    out = {}
    for name, grid in grids.items():
        tab, sensor = parity_sensor(128, 128, 2.0, grid)
        for gate in GATES:
            kw = dict(MATCH_DEFAULTS, rotations=3, min_points=4096, min_score=gate, min_gain=gate)
            out["%s, gates %d" % (name, gate)] = dict(tab=tab, H=128, W=128, res=0.1, kw=kw, sensors=[sensor])
    tab, sensor = parity_sensor(64, 64, 2.45, np.full((64, 64), -32768, np.int16))
    out["every candidate negative"] = dict(tab=tab, H=64, W=64, res=0.1, sensors=[sensor],
                                           kw=dict(MATCH_DEFAULTS, reach=8, rotations=3, min_points=1, min_score=0, min_gain=0))
    return out


def equal_cases():
    """An empty grid at the largest search (35 937 equal candidates: the zero candidate wins), and a wall painted one
    cell off under 33 rotations that are all the same (rot_step = 0: 33 tied candidates per translation, kappa = 0 wins)."""
    biggest = dict(reach=16, rotations=33, min_points=0, min_score=0, min_gain=0)
    rule = lambda kw, sensor: dict(tab=axis_beams(), H=RULE_H, W=RULE_W, res=RULE_RES,
                                   kw=dict(MATCH_DEFAULTS, max_range=3.0, **kw), sensors=[sensor])
    room = room_case(86, 450, 64, 128, scans=2, offsets=((0.1, 0.1, 0.01),))
    room["sensors"][0]["grid"] = np.zeros((64, 128), np.int16)
    tied = dict(rotations=33, rot_step=0.0, min_points=1, min_score=1, min_gain=1)
    return {"empty grid, axis beams": rule(biggest, _sensor(BASE_RANGES, np.zeros((RULE_H, RULE_W), np.int16))),
            "empty grid, room": with_search(room, **biggest),
            "33 equal rotations, reach 4": rule(dict(tied, reach=4), _sensor(BASE_RANGES, painted([(0, 1)]))),
            "33 equal rotations, reach 16": rule(dict(tied, reach=16), _sensor(BASE_RANGES, painted([(-1, 0)])))}


def moved_to(case, M):
    """The case with every sensor's world moved by (M, M): origin, pose and the terms of the pose."""
    out = dict(case, sensors=[])
    for s in case["sensors"]:
        pose = s["pose"] + np.array([M, M, 0.0])
        rot, trans = pose_terms(pose)
        out["sensors"].append(dict(s, pose=pose, rot=rot.reshape(2, 2), trans=trans, origin=s["origin"] + M))
    return out


def far_and_small_cases():
    """The four coordinate magnitudes at the default search; N = 1; NaN, +inf and -inf in one element of rot, trans,
    origin and pose of sensor 0 (at its true pose) beside a healthy sensor that is 0.3 m off."""
    base = room_case(84, 450, 128, 128, offsets=((0.23, -0.17, 0.021),))
    out = {"origin near %g" % M: moved_to(base, M) for M in MAGNITUDES}
    few = dict(MATCH_DEFAULTS, max_range=3.0, min_points=1, min_score=1, min_gain=1)
    out["N 1"] = dict(tab=angle_table(1, np.radians(0.5)), H=RULE_H, W=RULE_W, res=RULE_RES, kw=few,
                      sensors=[_sensor([1.0], noise_grid(9))])
    pair = room_case(85, 450, 128, 128, sensors=2, offsets=((0.0, 0.0, 0.0), (0.23, -0.17, 0.021)))
    for f, field in enumerate(("rot", "trans", "origin", "pose")):
        for v, (name, value) in enumerate(NON_FINITE):
            case = copy.deepcopy(pair)
            a = case["sensors"][0][field]
            a.reshape(-1)[(f + v) % a.size] = value
            out["%s in %s" % (name, field)] = case
    return out


def match_cases():
    out = {}
    for family in (reach_cases, long_scan_cases, packing_cases, extreme_cases, equal_cases, far_and_small_cases):
        out.update(family())
    return out


@pytest.fixture(scope="module")
def matched():
    cases = match_cases()
    return cases, {k: run_case(c) for k, c in cases.items()}


def thinned(case, sensor):
    """The sensor with all but every s-th voting point's range set to NaN, s the smallest stride that keeps the literal
    loop under LITERAL_BUDGET steps -> (sensor, s)."""
    kw = case["kw"]
    votes = voting_points(sensor["ranges"], sensor.get("inst"), sensor.get("num_det"), sensor.get("det_cls"),
                          kw["cls_thresh"], kw["max_range"])
    per_point = kw["rotations"] * (2 * kw["reach"] + 1) ** 2
    stride = max(1, -(-int(votes.sum()) * per_point // LITERAL_BUDGET))
    if stride == 1:
        return sensor, 1
    ranges = sensor["ranges"].copy()
    drop = np.flatnonzero(votes)
    ranges[np.setdiff1d(drop, drop[::stride])] = NAN
    return dict(sensor, ranges=ranges), stride


def test_every_match_case_equals_the_literal_loops(matched):
    cases, want = matched
    whole = 0
    for name, case in cases.items():
        kw = case["kw"]
        table = rotation_table(kw["rot_step"], kw["rotations"])
        for s, o in zip(case["sensors"], want[name]):
            t, stride = thinned(case, s)
            if stride > 1:
                o = run_case(dict(case, sensors=[t]))[0]
            votes = voting_points(t["ranges"], t.get("inst"), t.get("num_det"), t.get("det_cls"), kw["cls_thresh"],
                                  kw["max_range"])
            lit = literal_scores(t["ranges"], case["tab"], t["rot"], t["trans"], t["grid"], t["origin"], case["res"],
                                 votes, table, kw["reach"])
            assert np.array_equal(o["scores"], lit) and o["scores"].dtype == np.int32, name
            assert o["votes"] == votes.sum(), name
            whole += stride == 1
    print("literal loops: %d cases, %d sensors checked whole, the rest thinned to %d steps" % (len(cases), whole, LITERAL_BUDGET))


def test_reaches_and_long_scans(matched):
    cases, want = matched
    reaches = sorted({c["kw"]["reach"] for k, c in cases.items() if k.startswith("reach ")})
    slices = sorted({max(1, 256 // (2 * R + 1) ** 2) for R in reaches}, reverse=True)
    assert reaches == list(range(17)) and slices == [256, 28, 10, 5, 3, 2, 1]
    moved = {k: int(want[k][0]["moved"]) for k in cases if k.startswith("reach ")}
    assert sum(moved.values()) >= 20 and not moved["reach 0, 1 rotations"]
    for R, K in ((5, 33), (16, 33)):
        assert want["reach %d, 33 rotations" % R][0]["scores"].shape == (33, 2 * R + 1, 2 * R + 1)
    for name, N, T in (("N 4096, reach 8", 4096, 17), ("N 4096, reach 16", 4096, 33), ("N 513, reach 16", 513, 33)):
        o = want[name][0]
        assert len(cases[name]["sensors"][0]["ranges"]) == N and o["scores"].shape == (3, T, T) and o["votes"] > N // 2
        assert o["moved"], name
    print("reaches run: %s at 1 and 3 rotations (slices %s), 33 rotations at 5 and 16; moved in %d of %d; N 4096 at reach "
          "8 and 16, N 513 at reach 16" % (reaches, slices, sum(moved.values()), len(moved)))


def test_packing_cases_stage_points_on_all_four_borders(matched):
    cases, want = matched
    for H, W in PACK_SHAPES:
        name = "%d x %d" % (H, W)
        o = want[name][0]
        assert o["votes"] == PACK_N
        R = PACK_REACH
        for k in range(3):
            cells = o["cells"][k]
            bands = border_bands(cells, H, W, R)
            inside = int(((cells[:, 0] >= 0) & (cells[:, 0] < W) & (cells[:, 1] >= 0) & (cells[:, 1] < H)).sum())
            staged = int(((cells[:, 0] >= -R) & (cells[:, 0] < W + R) & (cells[:, 1] >= -R) & (cells[:, 1] < H + R)).sum())
            beyond = PACK_N - staged
            assert min(bands) >= 1 and inside >= 100 and beyond >= 1, (name, k, bands, inside, beyond)
            if k == 1:
                middle = (bands, inside, beyond)
        # a staged cell outside the grid adds nothing until a shift brings it in: the scores differ from shift to shift
        assert o["scores"].any() and (o["scores"][1] != o["scores"][1, R, R]).any()
        print("packing %s: staged points left / right / below / above the grid %s, inside %d, beyond reach %d (middle "
              "rotation)" % ((name,) + middle))


def test_score_extremes_and_the_gates_in_int64(matched):
    cases, want = matched
    top = X_N * 32767
    for gate in GATES:
        hi, lo, cb = (want["%s, gates %d" % (k, gate)][0] for k in ("all 32767", "all -32768", "checkerboard"))
        assert hi["votes"] == lo["votes"] == cb["votes"] == X_N
        assert (hi["scores"] == top).all() and hi["best"].tolist() == [0, 0, 0] and hi["score"].tolist() == [top, top]
        assert (hi["ok"], hi["moved"]) == (int(gate <= 32767), 0)                  # 32767 V: equality, ok
        assert (lo["scores"] == -X_N * 32768).all() and lo["best"].tolist() == [0, 0, 0] and (lo["ok"], lo["moved"]) == (0, 0)
        assert cb["score"].tolist() == [top, -top] and cb["best"].tolist() == [0, -1, 0]     # the lowest index at distance 1
        assert (cb["ok"], cb["moved"]) == ((1, 1) if gate <= 32767 else (0, 0))    # 2^31 - 1 times 4096 needs int64
    neg = want["every candidate negative"][0]
    assert (neg["scores"] < 0).all() and neg["votes"] == X_N and neg["score"][0] > neg["score"][1]
    assert neg["best"].tolist() != [0, 0, 0] and neg["score"][0] == neg["scores"].max() and (neg["ok"], neg["moved"]) == (0, 0)
    print("score extremes: +-%d reached; every candidate negative: best %d at %s against %d at the incoming pose"
          % (top, neg["score"][0], neg["best"].tolist(), neg["score"][1]))


def test_equal_candidates_far_coordinates_and_spoiled_terms(matched):
    cases, want = matched
    for name in ("empty grid, axis beams", "empty grid, room"):
        o = want[name][0]
        assert o["scores"].shape == (33, 33, 33) and not o["scores"].any()
        assert o["best"].tolist() == [0, 0, 0] and (o["ok"], o["moved"]) == (1, 0)
    for name, best in (("33 equal rotations, reach 4", [0, 0, 1]), ("33 equal rotations, reach 16", [0, -1, 0])):
        o = want[name][0]
        T, (_, dy, dx) = o["scores"].shape[1], best
        assert (o["scores"][:, T // 2 + dy, T // 2 + dx] == 120).all() and o["scores"].max() == 120
        assert o["best"].tolist() == best and o["moved"]
    near = want["origin near 0"][0]
    for M in MAGNITUDES:
        o = want["origin near %g" % M][0]
        s = cases["origin near %g" % M]["sensors"][0]
        assert abs(s["origin"][0] - M) < 10.0 and o["moved"] and o["votes"] == near["votes"]
    assert want["N 1"][0]["votes"] == 1 and want["N 1"][0]["scores"].any()
    for field in ("rot", "trans", "origin", "pose"):
        for value, _ in NON_FINITE:
            name = "%s in %s" % (value, field)
            spoiled, healthy = want[name]
            s = cases[name]["sensors"][0]
            assert not spoiled["moved"] and spoiled["pose"].tobytes() == s["pose"].tobytes(), name
            assert spoiled["trans"].tobytes() == s["trans"].tobytes() and not spoiled["correction"].any()
            assert field == "pose" or not spoiled["scores"].any(), name
            assert healthy["moved"], name
    print("all-equal candidates at 33 x 33 x 33: the zero candidate; four magnitudes moved alike; 12 spoiled sensors stay")
