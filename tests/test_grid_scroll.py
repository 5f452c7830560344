"""The scrolling occupancy grid (pof_grid_scroll, N14) without a GPU: ``grid_scroll_oracle`` is the NumPy restatement of
the comment in include/pof_abi.h, checked here on scenes whose numbers are exact (res = 0.125, origins on multiples of
it, grids in which every cell holds a value of its own, and a literal Python loop over the cells), and on ray-cast rooms
for what the stage is good for: a window that scrolls holds the cells a fixed map of the whole world holds, a sensor
that drives out of a fixed grid keeps its map, and the scan-to-grid match works across a scroll.
tests/test_grid_scroll_gpu.py imports the restatement and the scenes and holds the device to them bit for bit.

The stage has one float64 expression per axis, N12's point_cell arithmetic at the sensor position -- a subtraction, a
true division and a floor, each correctly rounded in NumPy and on the device alike -- and integers behind it: there is
no ambiguous scene and no tolerance."""
import inspect
import os
import re

import numpy as np
import pytest

from test_grid_map import DEFAULTS as MAP_DEFAULTS, grid_map_oracle
from test_grid_match import (CELL, DEFAULTS as MATCH_DEFAULTS, QUALITY_SEEDS as MATCH_SEEDS, SPOILED, advance, drive,
                             grid_match_oracle, pose_terms, reckon)
from test_scan_match import angle_table, make_room, match_oracle, ray_cast

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 64
CAP_CELL, CAP_OFFSET = 2.0 ** 30, 2 ** 20
RES = 0.125


# ---------------------------------------------------------------- restatement of the device rule, one sensor
def default_margin(H, W):
    """A quarter of the shorter side, rounded down to a multiple of 64."""
    return min(H, W) // 4 // TILE * TILE


def margin_bound(H, W):
    """The largest margin the entry point takes: a re-centred sensor stays outside it."""
    return TILE * ((min(H, W) // TILE - 1) // 2)


def axis_shift(t, o, res, margin, side, off):
    """The shift of one axis in tiles, by the header's words."""
    with np.errstate(all="ignore"):
        c = np.floor((np.float64(t) - np.float64(o)) / np.float64(res))        # a true division
    if not np.isfinite(c) or abs(c) >= CAP_CELL:
        return 0
    c = int(c)
    if margin <= c < side - margin:
        return 0
    s = c // TILE - (side // TILE) // 2                                        # Python's // floors
    return 0 if abs(int(off) + s) > CAP_OFFSET else s


def shifted(grid, sx, sy):
    """grid'[iy][ix] = grid[iy + 64 s_y][ix + 64 s_x] where that cell exists, else 0."""
    H, W = grid.shape
    out = np.zeros_like(grid)
    dx, dy = TILE * sx, TILE * sy
    x0, x1, y0, y1 = max(0, -dx), min(W, W - dx), max(0, -dy), min(H, H - dy)
    if x0 < x1 and y0 < y1:
        out[y0:y1, x0:x1] = grid[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def grid_scroll_oracle(trans, grid, origin, base, offset, res, margin=None):
    """One call for one sensor.  trans [2]; grid [H,W] int16, origin [2] float64 and offset [2] int32 are UPDATED IN
    PLACE (and keep their bits without a shift), base [2] is read.  -> dict(shift [2] int32, scrolled uint8)."""
    H, W = grid.shape
    margin = default_margin(H, W) if margin is None else margin
    sx = axis_shift(trans[0], origin[0], res, margin, W, offset[0])
    sy = axis_shift(trans[1], origin[1], res, margin, H, offset[1])
    if sx or sy:
        grid[...] = shifted(grid, sx, sy)
        offset += np.array([sx, sy], np.int32)
        origin[...] = np.asarray(base, np.float64) + (TILE * offset).astype(np.float64) * np.float64(res)
    return dict(shift=np.array([sx, sy], np.int32), scrolled=np.uint8(bool(sx or sy)))


def literal_shift(grid, sx, sy):
    """The cell rule as the header words it, one Python loop per index: for the small rule scenes only."""
    H, W = grid.shape
    out = np.zeros_like(grid)
    for iy in range(H):
        for ix in range(W):
            y, x = iy + TILE * sy, ix + TILE * sx
            if 0 <= y < H and 0 <= x < W:
                out[iy, ix] = grid[y, x]
    return out


# ---------------------------------------------------------------- rule scenes: exact numbers
def numbered(H, W, seed=0):
    """A grid in which every cell holds a value of its own (H W <= 65536)."""
    return (np.random.default_rng(seed).permutation(H * W).reshape(H, W) - 32768).astype(np.int16)


def at_cell(origin, cx, cy, res=RES):
    """The middle of cell (cx, cy) of the grid at ``origin``: exact for res = 0.125 and origins on multiples of it."""
    return np.array([origin[0] + (cx + 0.5) * res, origin[1] + (cy + 0.5) * res], np.float64)


def _sensor(H, W, steps, origin=(-8.0, -4.0), offset=(0, 0), base=None, seed=0):
    """A sensor of a scene: its grid, origin, base, offset and the positions of its calls, given as cells (cx, cy) of
    the grid as it stands at that call (or as a position, a float64 [2] array)."""
    origin = np.asarray(origin, np.float64)
    base = origin - (TILE * np.asarray(offset, np.float64)) * RES if base is None else np.asarray(base, np.float64)
    return dict(grid=numbered(H, W, seed), origin=origin, base=base, offset=np.asarray(offset, np.int32), steps=steps)


def _scene(H, W, margin, *sensors, res=RES):
    return dict(H=H, W=W, margin=margin, res=res, sensors=list(sensors))


MID_X, MID_Y = 8.0625, 12.0625                                 # the middle of a 256 x 256 grid at (-8, -4)
BIG = TILE * (CAP_OFFSET + 2)                                  # 256 x 256: the cell whose scroll is offset 2^20 exactly


def rule_scenes():
    """-> {name: scene}; a scene is dict(H, W, margin, res, sensors=[dict(grid, origin, base, offset, steps)]), all
    sensors of a scene with the same number of steps.  ``EXPECTED`` holds the shifts."""
    mid64, mid128, mid256 = (32, 32), (100, 70), (130, 140)
    return {
        # 64 x 64: one tile, the margin can only be 0, any scroll empties the grid
        "64 low x": _scene(64, 64, 0, _sensor(64, 64, [(0, 32), (-1, 32)])),
        "64 high x": _scene(64, 64, 0, _sensor(64, 64, [(63, 32), (64, 32)])),
        "64 low y": _scene(64, 64, 0, _sensor(64, 64, [(32, 0), (32, -1)])),
        "64 high y": _scene(64, 64, 0, _sensor(64, 64, [(32, 63), (32, 64)])),
        # 128 x 192: TH = 2, TW = 3, margin 0 (its bound): a scroll only outside the grid
        "128x192 low x": _scene(128, 192, 0, _sensor(128, 192, [(0, 70), (-1, 70)])),
        "128x192 high x": _scene(128, 192, 0, _sensor(128, 192, [(191, 70), (192, 70)])),
        "128x192 low y": _scene(128, 192, 0, _sensor(128, 192, [(100, 0), (100, -1)])),
        "128x192 high y": _scene(128, 192, 0, _sensor(128, 192, [(100, 127), (100, 128)])),
        "128x192 both": _scene(128, 192, 0, _sensor(128, 192, [mid128, (255, 128)])),
        # 256 x 256, margin 64 (the default and the bound): c = margin - 1 | margin, W - margin - 1 | W - margin
        "256 low x": _scene(256, 256, 64, _sensor(256, 256, [(64, 140), (63, 140)])),
        "256 high x": _scene(256, 256, 64, _sensor(256, 256, [(191, 140), (192, 140)])),
        "256 low y": _scene(256, 256, 64, _sensor(256, 256, [(130, 64), (130, 63)])),
        "256 high y": _scene(256, 256, 64, _sensor(256, 256, [(130, 191), (130, 192)])),
        "256 both": _scene(256, 256, 64, _sensor(256, 256, [(191, 64), (192, 63)])),
        "256 margin 0": _scene(256, 256, 0, _sensor(256, 256, [(0, 255), (255, 0), (256, -1)])),
        # a shift of the grid's size and more: everything is unknown
        "256 clears": _scene(256, 256, 64, _sensor(256, 256, [(128 + 4 * 64, 140)]), _sensor(256, 256, [(130, -900)], seed=1)),
        # nothing to go by: NaN, inf, a cell at 2^30 (2^30 - 1 would be a shift past the offset cap: not made either)
        "256 spoiled": _scene(256, 256, 64, *[_sensor(256, 256, [np.array(t, np.float64)], seed=k) for k, t in enumerate(
            [(np.nan, MID_Y), (MID_X, np.inf), (-np.inf, np.nan), (-8.0 + 2.0 ** 30 * RES, MID_Y),
             (MID_X, -4.0 - 2.0 ** 30 * RES), (-8.0 + (2.0 ** 30 - 1) * RES, MID_Y)])]),
        # the offset cap: 2^20 is reached, 2^20 + 1 is not made, on either side, per axis
        "256 cap": _scene(256, 256, 64,
                          _sensor(256, 256, [(BIG, 140), (192, 140)]),
                          _sensor(256, 256, [(BIG + 64, 140), (130, 192)], seed=1),
                          _sensor(256, 256, [(130, 63 - BIG + 256), (130, 63)], seed=2),
                          _sensor(256, 256, [(192 + 64, 192), mid256], offset=(CAP_OFFSET - 1, 0), seed=3),
                          _sensor(256, 256, [(192, 140), (63, 140)], offset=(CAP_OFFSET - 1, 1 - CAP_OFFSET), seed=4)),
        # away and back: +1, -2, +1 tiles in x; the origin is not on the cell raster and res is not a power of two
        "256 away and back": _scene(256, 256, 64, _sensor(256, 256, [mid256, (192, 140), (63, 140), (192, 140), mid256],
                                                         origin=(0.3, -0.7)), res=0.1),
        # a mixed batch in 128 x 192: sensors 0 and 2 stay, 1 and 3 scroll (3 in both axes)
        "128x192 mixed": _scene(128, 192, 0, _sensor(128, 192, [mid128, (0, 0)]), _sensor(128, 192, [mid128, (192, 5)], seed=1),
                                _sensor(128, 192, [(191, 127), mid128], seed=2),
                                _sensor(128, 192, [mid128, (200, 130)], seed=3)),
        "64 mid": _scene(64, 64, 0, _sensor(64, 64, [mid64])),
    }


# what every call of every sensor of a scene must answer: the shifts (x, y) in tiles
EXPECTED = {
    "64 low x": [[(0, 0), (-1, 0)]], "64 high x": [[(0, 0), (1, 0)]],
    "64 low y": [[(0, 0), (0, -1)]], "64 high y": [[(0, 0), (0, 1)]],
    "128x192 low x": [[(0, 0), (-2, 0)]], "128x192 high x": [[(0, 0), (2, 0)]],
    "128x192 low y": [[(0, 0), (0, -2)]], "128x192 high y": [[(0, 0), (0, 1)]],
    "128x192 both": [[(0, 0), (2, 1)]],
    "256 low x": [[(0, 0), (-2, 0)]], "256 high x": [[(0, 0), (1, 0)]],
    "256 low y": [[(0, 0), (0, -2)]], "256 high y": [[(0, 0), (0, 1)]],
    "256 both": [[(0, 0), (1, -2)]],
    "256 margin 0": [[(0, 0), (0, 0), (2, -3)]],
    "256 clears": [[(4, 0)], [(0, -17)]],
    "256 spoiled": [[(0, 0)]] * 6,
    "256 cap": [[(CAP_OFFSET, 0), (0, 0)], [(0, 0), (0, 1)], [(0, -CAP_OFFSET), (0, 0)], [(0, 1), (0, 0)],
                [(1, 0), (-2, 0)]],
    "256 away and back": [[(0, 0), (1, 0), (-2, 0), (1, 0), (0, 0)]],
    "128x192 mixed": [[(0, 0), (0, 0)], [(0, 0), (2, 0)], [(0, 0), (0, 0)], [(0, 0), (2, 1)]],
    "64 mid": [[(0, 0)]],
}


def step_trans(sensor, step, origin, res):
    """The position of a call: a cell (cx, cy) of the grid at ``origin``, or the position itself."""
    return step if isinstance(step, np.ndarray) else at_cell(origin, step[0], step[1], res)


def run_scene(scene):
    """The restatement over every sensor of a scene -> per sensor a list with one dict per call: trans (the input),
    shift, scrolled, and copies of grid, origin and offset behind the call."""
    out = []
    for s in scene["sensors"]:
        grid, origin, offset = s["grid"].copy(), s["origin"].copy(), s["offset"].copy()
        calls = []
        for step in s["steps"]:
            trans = step_trans(s, step, origin, scene["res"])
            o = grid_scroll_oracle(trans, grid, origin, s["base"], offset, scene["res"], scene["margin"])
            calls.append(dict(o, trans=trans, grid=grid.copy(), origin=origin.copy(), offset=offset.copy()))
        out.append(calls)
    return out


@pytest.fixture(scope="module")
def rules():
    return {k: run_scene(s) for k, s in rule_scenes().items()}


def test_every_scene_has_its_expected_shifts(rules):
    assert set(EXPECTED) == set(rules)
    for name, sensors in rules.items():
        got = [[tuple(int(v) for v in c["shift"]) for c in calls] for calls in sensors]
        assert got == [list(e) for e in EXPECTED[name]], (name, got)
        for calls in sensors:
            for c in calls:
                assert c["scrolled"] == (1 if c["shift"].any() else 0) and c["shift"].dtype == np.int32


def test_every_rule_scene_equals_the_literal_loop(rules):
    for name, scene in rule_scenes().items():
        for s, calls in zip(scene["sensors"], rules[name]):
            grid = s["grid"]
            assert len(np.unique(grid)) == grid.size                           # every cell holds a value of its own
            for c in calls:
                sx, sy = (int(v) for v in c["shift"])
                if TILE * abs(sx) >= grid.shape[1] or TILE * abs(sy) >= grid.shape[0]:
                    want = np.zeros_like(grid)                                 # a shift of the grid's size or more
                else:
                    want = literal_shift(grid, sx, sy) if (sx or sy) else grid
                assert np.array_equal(c["grid"], want), name
                grid = c["grid"]


def test_the_trigger_flips_at_the_margin_and_re_centres(rules):
    for name in ("256 low x", "256 high x", "256 low y", "256 high y", "256 both", "128x192 high x", "128x192 both"):
        scene = rule_scenes()[name]
        for s, calls in zip(scene["sensors"], rules[name]):
            first, last = calls[0], calls[-1]
            # one cell short of the margin: every bit is kept
            assert first["grid"].tobytes() == s["grid"].tobytes() and first["origin"].tobytes() == s["origin"].tobytes()
            assert not first["offset"].any() and not first["scrolled"] and last["scrolled"]
            # behind the scroll the sensor stands on the middle tile of each axis that moved, outside the margin
            c = np.floor((last["trans"] - last["origin"]) / scene["res"]).astype(int)
            for axis, side in ((0, scene["W"]), (1, scene["H"])):
                if last["shift"][axis]:
                    assert c[axis] // TILE == (side // TILE) // 2, name
                    assert scene["margin"] <= c[axis] < side - scene["margin"], name
    # the numbers of one of them: 256 x 256 at (-8, -4), the sensor in cell (192, 140) -> one tile in x
    o = rules["256 high x"][0][-1]
    assert o["origin"].tolist() == [0.0, -4.0] and o["offset"].tolist() == [1, 0]
    g0 = rule_scenes()["256 high x"]["sensors"][0]["grid"]
    assert np.array_equal(o["grid"][:, :192], g0[:, 64:]) and not o["grid"][:, 192:].any()
    o = rules["256 both"][0][-1]
    assert o["origin"].tolist() == [0.0, -20.0] and o["offset"].tolist() == [1, -2]
    assert np.array_equal(o["grid"][128:, :192], g0[:128, 64:]) and not o["grid"][:128].any() and not o["grid"][:, 192:].any()


def test_one_tile_and_full_size_shifts_empty_the_grid(rules):
    for name in ("64 low x", "64 high x", "64 low y", "64 high y"):
        first, last = rules[name][0]
        assert first["grid"].any() and not last["grid"].any() and last["scrolled"], name
    for calls in rules["256 clears"]:
        assert not calls[0]["grid"].any() and calls[0]["scrolled"]
    assert rules["256 clears"][0][0]["origin"].tolist() == [-8.0 + 4 * 8.0, -4.0]
    assert rules["256 clears"][1][0]["origin"].tolist() == [-8.0, -4.0 - 17 * 8.0]
    # margin 0: cells 0 and 255 are inside; (256, -1) is outside on both axes and leaves one tile row of two columns
    last = rules["256 margin 0"][0][-1]
    assert last["offset"].tolist() == [2, -3] and last["grid"][192:, :128].all() and not last["grid"][:192].any()


def test_spoiled_positions_and_the_caps_scroll_nothing(rules):
    scene = rule_scenes()["256 spoiled"]
    for s, calls in zip(scene["sensors"], rules["256 spoiled"]):
        c = calls[0]
        assert c["grid"].tobytes() == s["grid"].tobytes() and c["origin"].tobytes() == s["origin"].tobytes()
        assert not c["offset"].any() and not c["scrolled"]
    cap = rules["256 cap"]
    assert cap[0][0]["offset"].tolist() == [CAP_OFFSET, 0] and cap[0][0]["origin"].tolist() == [-8.0 + 2.0 ** 23, -4.0]
    assert cap[0][1]["offset"].tolist() == [CAP_OFFSET, 0] and not cap[0][1]["scrolled"]     # + 1 more is not made
    # one axis past the cap keeps that axis only: the other one still scrolls
    assert cap[1][0]["offset"].tolist() == [0, 0] and cap[1][1]["offset"].tolist() == [0, 1]
    assert cap[2][0]["offset"].tolist() == [0, -CAP_OFFSET] and not cap[2][1]["scrolled"]
    assert cap[3][0]["offset"].tolist() == [CAP_OFFSET - 1, 1]                 # x would be 2^20 + 1
    assert cap[4][0]["offset"].tolist() == [CAP_OFFSET, 1 - CAP_OFFSET] and cap[4][1]["offset"].tolist() == [CAP_OFFSET - 2, 1 - CAP_OFFSET]


def test_away_and_back_gives_the_origin_its_bits_back(rules):
    scene = rule_scenes()["256 away and back"]
    s, calls = scene["sensors"][0], rules["256 away and back"][0]
    assert [c["offset"].tolist() for c in calls] == [[0, 0], [1, 0], [-1, 0], [0, 0], [0, 0]]
    assert calls[3]["origin"].tobytes() == s["origin"].tobytes() == calls[4]["origin"].tobytes()
    # not what accumulating gives: 0.3 + 6.4 - 12.8 + 6.4 in float64
    assert calls[1]["origin"][0] == 0.3 + 64.0 * 0.1 and ((0.3 + 6.4) - 12.8) + 6.4 != 0.3
    # +1: columns 64.. move to 0..; -2: columns 0..127 of that move to 128..; +1: those move to 64..191
    back = calls[3]["grid"]
    assert np.array_equal(back[:, 64:192], s["grid"][:, 64:192])               # the cells that never left
    assert not back[:, :64].any() and not back[:, 192:].any()


def test_a_mixed_batch_keeps_every_bit_of_the_sensors_that_stay(rules):
    scene = rule_scenes()["128x192 mixed"]
    for b, (s, calls) in enumerate(zip(scene["sensors"], rules["128x192 mixed"])):
        last = calls[-1]
        if b in (0, 2):
            assert last["grid"].tobytes() == s["grid"].tobytes() and last["origin"].tobytes() == s["origin"].tobytes()
            assert last["offset"].tobytes() == s["offset"].tobytes() and not last["scrolled"]
        else:
            assert last["scrolled"] and last["offset"].any()
    both = rules["128x192 mixed"][3][-1]
    g0 = scene["sensors"][3]["grid"]
    assert np.array_equal(both["grid"][:64, :64], g0[64:, 128:]) and not both["grid"][64:].any() and \
        not both["grid"][:, 64:].any()


def test_margins():
    assert [default_margin(s, s) for s in (64, 128, 256, 512, 1024, 2048)] == [0, 0, 64, 128, 256, 512]
    assert default_margin(128, 192) == 0 and default_margin(512, 256) == 64
    for H, W in ((64, 64), (128, 192), (256, 256), (512, 512), (2048, 2048), (512, 256)):
        assert default_margin(H, W) <= margin_bound(H, W)
    assert [margin_bound(s, s) for s in (64, 128, 192, 256, 512)] == [0, 0, 64, 64, 192]


def device_scenes():
    """-> {name: scene}: what tests/test_grid_scroll_gpu.py runs beside the rule scenes -- one sensor in 2048 x 2048
    with a one-tile and a full-size shift: cell indices past 2^21 per sensor, and values that are not all distinct."""
    def big(steps, seed):
        s = _sensor(64, 64, steps, origin=(-128.0, -128.0))
        s["grid"] = np.random.default_rng(seed).integers(-40, 71, (2048, 2048)).astype(np.int16)
        return s
    return {"2048 one tile": _scene(2048, 2048, 512, big([(1024, 1024), (1536, 511)], 5)),
            "2048 full size": _scene(2048, 2048, 512, big([(1024 + 2048, 1024 - 2048)], 6))}


def test_device_scenes_reach_their_shapes():
    got = {k: run_scene(s) for k, s in device_scenes().items()}
    one = got["2048 one tile"][0]
    assert one[0]["shift"].tolist() == [0, 0] and one[1]["shift"].tolist() == [8, -9]
    assert one[1]["grid"][9 * 64:, :-8 * 64].any() and not one[1]["grid"][:9 * 64].any() and not one[1]["grid"][:, -8 * 64:].any()
    full = got["2048 full size"][0]
    assert full[0]["shift"].tolist() == [32, -32] and not full[0]["grid"].any()


# ---------------------------------------------------------------- window equals map
def long_room(rng, stretch):
    """tests/test_scan_match.make_room stretched along x, and a lane y = const through it that keeps 0.4 m clear of
    every box: -> (segments [M,2,2], half length, lane y)."""
    segs = make_room(rng)
    segs[..., 0] *= stretch
    hx, hy = segs[:4, :, 0].max(), segs[:4, :, 1].max()
    boxes = segs[4:].reshape(-1, 4, 2, 2)
    lo, hi = boxes[..., 1].min(axis=(1, 2)) - 0.4, boxes[..., 1].max(axis=(1, 2)) + 0.4
    for y in sorted(np.linspace(-hy + 1.0, hy - 1.0, 41), key=abs):
        if not ((lo < y) & (y < hi)).any():
            return segs, hx, float(y)
    raise AssertionError("no free lane: re-seed")


def straight_drive(seed, length, step, stretch=6.0, noise=0.01, N=450):
    """A sensor driven along the lane of a long room, heading along +x with a small weave: -> (tab, scans float32 [T,N]
    with ``noise`` m of range noise and a 225 degree view, poses [T,3])."""
    rng = np.random.default_rng(seed)
    tab = angle_table(N, np.radians(225.0) / N)
    segs, hx, y = long_room(rng, stretch)
    assert 2.0 * hx - 3.0 >= length, "the room is too short: re-seed"
    T = int(np.ceil(length / step)) + 1
    poses = np.zeros((T, 3))
    poses[:, 0] = -hx + 1.5 + step * np.arange(T) + rng.uniform(-0.02, 0.02, T)
    poses[:, 1] = y + rng.uniform(-0.05, 0.05, T)
    poses[:, 2] = rng.uniform(-0.05, 0.05, T)
    scans = np.stack([(ray_cast(segs, p, tab[:N]) + rng.normal(0.0, 1.0, N) * noise).astype(np.float32) for p in poses])
    return tab, scans, poses


WINDOW_SEEDS = (21, 22)
WINDOW, WORLD, WINDOW_RANGE = 128, 1024, 5.0


def window_and_map(seed):
    """A 128 x 128 window that scrolls and a fixed 1024 x 1024 map of the same cells, driven with the same scans at the
    same poses.  -> (compared cells, mismatches among them, known cells of the last window, the compared ones among
    them, cells inside the window at every scan, scrolls)."""
    tab, scans, poses = straight_drive(seed, 27.0, 1.0, stretch=4.5)
    kw = dict(MAP_DEFAULTS, max_range=WINDOW_RANGE)
    # the base origin on a multiple of res, the sensor in the middle of the window; the map's origin a whole number of
    # cells from it
    base = np.floor(poses[0, :2] / RES) * RES - 0.5 * RES * WINDOW
    world_origin = base - RES * np.array([64.0, (WORLD - WINDOW) // 2])
    win, origin, offset = np.zeros((WINDOW, WINDOW), np.int16), base.copy(), np.zeros(2, np.int32)
    world, touched = np.zeros((WORLD, WORLD), np.int16), np.zeros((WORLD, WORLD), bool)
    # a cell of the window counts while the window has seen everything the map has seen of it: it has been inside at
    # every scan, or it scrolled in before any scan touched it and has been inside since
    counts = np.ones((WINDOW, WINDOW), bool)
    always = np.ones((WINDOW, WINDOW), bool)
    scrolls = 0
    for scan, pose in zip(scans, poses):
        rot, trans = pose_terms(pose)
        o = grid_scroll_oracle(trans, win, origin, base, offset, RES, 0)
        if o["scrolled"]:
            scrolls += 1
            sx, sy = (int(v) for v in o["shift"])
            x0, y0 = (int(v) for v in np.rint((origin - world_origin) / RES))
            counts = shifted(counts.astype(np.int16), sx, sy).astype(bool) | \
                (shifted(np.ones_like(win), sx, sy) == 0) & ~touched[y0:y0 + WINDOW, x0:x0 + WINDOW]
            always = shifted(always.astype(np.int16), sx, sy).astype(bool)
        grid_map_oracle(scan, tab, rot, trans, win, origin, RES, **kw)
        before = world.copy()
        grid_map_oracle(scan, tab, rot, trans, world, world_origin, RES, **kw)
        touched |= world != before
    x0, y0 = (int(v) for v in np.rint((origin - world_origin) / RES))
    assert 0 <= x0 <= WORLD - WINDOW and 0 <= y0 <= WORLD - WINDOW
    same = win == world[y0:y0 + WINDOW, x0:x0 + WINDOW]
    known = win != 0
    return int(counts.sum()), int((counts & ~same).sum()), int(known.sum()), int((known & counts).sum()), \
        int(always.sum()), scrolls


def test_the_window_holds_the_cells_of_a_fixed_map():
    """A 128 x 128 grid has two tiles per side and takes margin 0 only: a scroll moves it by half its size or empties
    it, so no cell is inside the window at every scan of a drive with three scrolls (the count is printed: 0).  The
    comparison therefore covers every cell for which the window has seen what the map has seen -- inside at every scan,
    or scrolled in before any scan had touched it and inside since -- which holds the former and is not empty:
    max_range = 5 m keeps a scan from touching the far half of what scrolls in.  Measured, seeds 21 and 22: 3 scrolls
    each, every compared cell equal (cap 0), the compared share of the last window's known cells in the printout."""
    for seed in WINDOW_SEEDS:
        compared, wrong, known, covered, always, scrolls = window_and_map(seed)
        print("seed %d: %d scrolls; %d cells compared, %d differ; %d of the last window's %d known cells compared; %d "
              "cells inside at every scan" % (seed, scrolls, compared, wrong, covered, known, always))
        assert scrolls >= 3 and wrong == 0, seed
        assert known > 0 and covered / known > 0.0, seed


# ---------------------------------------------------------------- what the stage is good for
QUALITY_SEEDS = (31, 32, 33)
QUALITY_LENGTH, QUALITY_STEP = 31.25, 1.25


def _quality(seed):
    """A straight drive of 31.25 m with the defaults (0.1 m cells, max_range 20 m), three maps driven with the same
    scans at the same poses and centred on the first one: 256 x 256 fixed, 256 x 256 scrolling with the default margin,
    2048 x 2048 fixed.  -> per map (endpoints of the last scan inside the grid, the share of them on cells with a prior
    >= hit), and the scrolls."""
    tab, scans, poses = straight_drive(seed, QUALITY_LENGTH, QUALITY_STEP)
    out, scrolls = {}, 0
    for name, size, scroll in (("fixed", 256, False), ("scrolling", 256, True), ("large", 2048, False)):
        base = poses[0, :2] - 0.5 * CELL * size
        grid, origin, offset = np.zeros((size, size), np.int16), base.copy(), np.zeros(2, np.int32)
        for scan, pose in zip(scans, poses):
            rot, trans = pose_terms(pose)
            if scroll:
                scrolls += int(grid_scroll_oracle(trans, grid, origin, base, offset, CELL)["scrolled"])
            last = grid_map_oracle(scan, tab, rot, trans, grid, origin, CELL)
        seen = last["point_cell"] >= 0
        out[name] = (int(seen.sum()), float((last["point_prior"][seen] >= MAP_DEFAULTS["hit"]).mean()) if seen.any() else 0.0)
    return out, scrolls


def test_quality_on_a_long_drive():
    """Measured with this restatement (recorded in DESIGN.md 8, N14), seeds 31-33, 26 scans 1.25 m apart: without the
    stage the last scan has no endpoint inside the 256 x 256 grid in any seed; with it 317-357 of 450, of which 0.504 /
    0.972 / 0.814 lie on cells with a prior >= hit; in a fixed 2048 x 2048 grid 403-426 endpoints, 0.484 / 0.923 / 0.789
    of them.  The share itself is the room's (how much of the last scan a scan 1.25 m earlier saw); the window is ahead
    of the large grid by 0.020 / 0.049 / 0.025 because the endpoints it leaves out are the far ones, which are the new
    ones.  The bound: not below the large grid's share by more than the spread of that difference over the seeds,
    0.049 - 0.020 = 0.029."""
    for seed in QUALITY_SEEDS:
        q, scrolls = _quality(seed)
        print("seed %d: %d scrolls; endpoints inside / share known: fixed 256 %d / %.3f, scrolling 256 %d / %.3f, "
              "fixed 2048 %d / %.3f" % ((seed, scrolls) + q["fixed"] + q["scrolling"] + q["large"]))
        assert q["fixed"][0] == 0 and scrolls >= 3, seed       # the sensor has left a grid that stays
        assert q["scrolling"][0] > 0 and q["large"][0] > 0, seed
        assert q["scrolling"][1] >= q["large"][1] - 0.029, seed


# ---------------------------------------------------------------- the scan-to-grid match across a scroll
def reckon_scrolling(tab, scans, start, origin, size=256):
    """tests/test_grid_match.reckon with the stage in its place of the streaming chain: the scan match and the pose
    launch, the scroll, the grid match, the grid update.  ``origin``: where the grid starts.
    -> (poses [T,3], the grid-match dicts, the scans at which the grid scrolled)."""
    pose, init = np.asarray(start, np.float64).copy(), None
    base, origin, offset = np.array(origin, np.float64), np.array(origin, np.float64), np.zeros(2, np.int32)
    grid, poses, outs, scrolled = np.zeros((size, size), np.int16), [], [], []
    for t, scan in enumerate(scans):
        if t > 0:
            m = match_oracle(scans[t - 1], scan, tab, init=init)
            init = m["motion"]
            if m["ok"]:
                pose = advance(pose, m["motion"])
        rot, trans = pose_terms(pose)
        if grid_scroll_oracle(trans, grid, origin, base, offset, CELL)["scrolled"]:
            scrolled.append(t)
        o = grid_match_oracle(scan, tab, rot, trans, pose, grid, origin, CELL, **MATCH_DEFAULTS)
        pose = o["pose"]
        grid_map_oracle(scan, tab, o["rot"], o["trans"], grid, origin, CELL)
        poses.append(pose.copy())
        outs.append(o)
    return np.array(poses), outs, scrolled


def _placed(reckoned, t, cells_inside, size=256):
    """The origin that puts the dead-reckoned position of scan ``t`` ``cells_inside`` cells (a fraction of a cell
    more) inside the default margin of the border the sensor drives towards, and in the middle of the other axis."""
    margin = default_margin(size, size)
    step = reckoned[-1, :2] - reckoned[0, :2]
    axis = int(np.argmax(np.abs(step)))
    cell = np.array([size // 2 + 0.5, size // 2 + 0.5])
    cell[axis] = size - margin - cells_inside + 0.01 if step[axis] > 0 else margin - 1 + cells_inside + 0.99
    return reckoned[t, :2] - cell * CELL


@pytest.mark.parametrize("where", ["four cells inside at the start", "the last scan in front of the lost pairs"])
def test_grid_match_recovers_across_a_scroll(where):
    """tests/test_grid_match.py's recovery scene (scan 13 all NaN: pairs (12, 13) and (13, 14) fail, scan 14 is
    corrected) in a 256 x 256 grid that scrolls with the default margin, placed so that the sensor starts four cells
    inside the margin and drives towards it.  The pose stands still over the lost pairs, so no scroll can fire between
    them and the correction; the second placement puts the scroll as close in front of them as a moving pose allows,
    at scan 12.  Asserted as that file does: ``moved`` fires at scan 14 and at no other, and the end error is at most
    a cell diagonal above the undisturbed sequence's.  Measured, seeds 11-14: the scroll fires at scans 4-5 with the
    first placement and at scan 12 with the second; end error 0.006-0.040 m, what that file measures without a scroll."""
    for seed in MATCH_SEEDS:
        tab, scans, truth = drive(seed)
        reckoned = reckon(tab, scans, truth[0], False)[0]      # dead reckoning alone: where the scrolls will be
        undisturbed = reckon(tab, drive(seed, spoil=False)[1], truth[0], False)[0]
        origin = _placed(reckoned, 0, 4) if where.startswith("four") else _placed(reckoned, SPOILED - 1, 0)
        poses, outs, scrolled = reckon_scrolling(tab, scans, truth[0], origin)
        fired = [t for t, o in enumerate(outs) if o["moved"]]
        err = float(np.hypot(*(poses[-1, :2] - truth[-1, :2])))
        err_undisturbed = float(np.hypot(*(undisturbed[-1, :2] - truth[-1, :2])))
        print("seed %d, %s: scrolled at scans %s, moved at scans %s, end error %.3f m (undisturbed %.3f m)"
              % (seed, where, scrolled, fired, err, err_undisturbed))
        assert len(scrolled) >= 1 and scrolled[0] <= SPOILED - 1, seed          # in front of the correction
        if not where.startswith("four"):
            assert scrolled == [SPOILED - 1], seed
        assert fired == [SPOILED + 1] and not outs[SPOILED]["ok"], seed
        assert err <= np.sqrt(2.0) * CELL + err_undisturbed, seed


# ---------------------------------------------------------------- surface
def test_records_and_settings_against_literal_tables():
    import torch
    from planar_optical_flow_amd import ops, streaming
    B, H, W = 2, 64, 128                                       # pairwise distinct: a transposed shape cannot pass
    f64, i32, i16, u8 = torch.float64, torch.int32, torch.int16, torch.uint8
    records = {
        "grid_scroll_state": ((B, H, W), "GridScrollState", (
            ("base", f64, (2, 2)), ("offset", i32, (2, 2)), ("scratch", i16, (2, 64, 128)))),
        "grid_scroll_buffers": ((B,), "GridScroll", (("shift", i32, (2, 2)), ("scrolled", u8, (2,)))),
    }
    for fn, (args, cls, fields) in records.items():
        rec = getattr(ops, fn)(*args, device="cpu")
        assert type(rec) is getattr(ops, cls) and type(rec).__name__ == cls, fn
        assert rec._fields == tuple(f for f, _, _ in fields), fn
        for (f, dtype, shape), t in zip(fields, rec):
            assert (t.dtype, tuple(t.shape), t.device.type) == (dtype, shape, "cpu"), (fn, f)
            assert not t.any(), (fn, f)
    assert ops.GridScrollState.persistent == ("base", "offset") and ops.GridScroll.persistent == ()
    assert ops.GridMapState._fields == ("grid", "origin")      # the grid's record stays what N12 declared
    # the settings: one source
    assert ops.stage_settings(ops.grid_scroll) == dict(res=ops.REQUIRED, margin=None)
    want = dict(margin=None)
    assert streaming.stage_defaults("grid_scroll") == want and streaming.stage_settings("grid_scroll", {}) == want
    assert streaming.stage_defaults("grid_scroll", 0.7, "keyframe") == want
    assert streaming.stage_settings("grid_scroll", dict(margin=64)) == dict(margin=64)
    for unknown in ("res", "size", "cls_thresh", "no_such_setting"):
        with pytest.raises(ValueError, match="unknown grid_scroll settings"):
            streaming.stage_settings("grid_scroll", {unknown: 1})
    # grid_map's dict holds what it held: the stage is an argument of its own
    assert "margin" not in streaming.stage_defaults("grid_map") and "scroll" not in streaming.stage_defaults("grid_map")
    assert [ops.grid_scroll_margin(s, s) for s in (64, 128, 256, 512, 2048)] == [default_margin(s, s) for s in (64, 128, 256, 512, 2048)]
    assert ops.grid_scroll_margin(128, 192) == 0 and ops.grid_scroll_margin(512, 256) == 64
    # a given margin is held to the entry point's bound, where the wrappers of the stage check their setting
    for H, W in ((64, 64), (128, 192), (256, 256), (512, 512), (512, 256)):
        bound = margin_bound(H, W)
        assert ops.grid_scroll_margin(H, W, bound) == bound and ops.grid_scroll_margin(H, W, 0) == 0
        for bad in (bound + 1, -1):
            with pytest.raises(ValueError):
                ops.grid_scroll_margin(H, W, bad)
    # grid_scroll_reset: base <- origin, offset <- 0, with tensor ops
    scroll = ops.grid_scroll_state(B, H, W, device="cpu")
    state = ops.grid_map_reset(ops.grid_map_state(B, H, W, device="cpu"), (1.5, -2.25))
    scroll.offset.fill_(7)
    assert ops.grid_scroll_reset(scroll, state) is not None
    assert scroll.base.tolist() == [[1.5, -2.25]] * 2 and not scroll.offset.any()


def test_header_binding_and_wrappers():
    import torch
    from planar_optical_flow_amd import _lib, ops
    from planar_optical_flow_amd.src.utils import utils
    from planar_optical_flow_amd.streaming import StreamingDetector
    text = open(os.path.join(REPO, "include", "pof_abi.h")).read()
    m = re.search(r"\bint\s+pof_grid_scroll\s*\(([^)]*)\)\s*;", text)
    assert m, "include/pof_abi.h does not declare pof_grid_scroll"
    params = [p.strip() for p in m.group(1).split(",")]
    restype, argtypes = _lib.SIGNATURES["pof_grid_scroll"]
    assert restype is _lib._i and len(argtypes) == len(params) == 14
    for p, t in zip(params, argtypes):
        want = _lib._p if "*" in p or p.startswith("pof_stream_t") else _lib._d if p.startswith("double") else _lib._i
        assert t is want, p
    # the records are unpacked positionally into the call: state, scroll, out in the header's order
    names = [re.sub(r".*[ *]", "", p) for p in params]
    assert names[6:13] == list(ops.GridMapState._fields + ops.GridScrollState._fields + ops.GridScroll._fields)
    assert "N14" in text and "scratch" in text and "#define POF_ABI_VERSION 1" in text
    for name in ("grid_scroll", "grid_scroll_buffers", "grid_scroll_state", "grid_scroll_reset"):
        assert callable(getattr(ops, name))
    p = inspect.signature(ops.grid_scroll).parameters
    assert list(p) == ["trans", "state", "scroll", "res", "margin", "out"]
    assert p["res"].kind is inspect.Parameter.KEYWORD_ONLY and p["res"].default is inspect.Parameter.empty
    assert p["margin"].default is None and p["out"].default is None
    assert inspect.signature(utils.OccupancyGrid.__init__).parameters["scroll"].default is None
    assert isinstance(utils.OccupancyGrid.offset, property)
    assert inspect.signature(StreamingDetector.__init__).parameters["grid_scroll"].default is None
    assert callable(StreamingDetector.grid_scroll)
    # no CPU path
    f64 = torch.float64
    state = ops.grid_map_state(1, 64, 64, device="cpu")
    scroll = ops.grid_scroll_state(1, 64, 64, device="cpu")
    with pytest.raises(TypeError):
        ops.grid_scroll(torch.zeros(1, 2, dtype=f64), state, scroll, res=0.1)
    with pytest.raises(TypeError):
        ops.grid_scroll(None, None, None, res=0.1)
    # the wrapper refuses wrong settings before it touches a device
    for bad in (dict(scroll=dict(margins=3)), dict(scroll=dict(res=0.1)), dict(scroll=dict(margin=128), size=256),
                dict(scroll=dict(margin=-1)), dict(scroll=dict(margin=64), size=128)):
        with pytest.raises(ValueError):
            utils.OccupancyGrid(np.zeros(4), **bad)


def test_entry_point_refuses_null_and_bad_arguments():
    import ctypes
    from planar_optical_flow_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "pof_grid_scroll")
    _, argtypes = _lib.SIGNATURES["pof_grid_scroll"]
    assert lib.pof_grid_scroll(*[None if t is _lib._p else 0 for t in argtypes]) == _lib.POF_E_BADARG
    assert lib.pof_grid_scroll(*[None if t is _lib._p else 1 for t in argtypes]) == _lib.POF_E_BADARG
    # every pointer given (never read: a refusal comes before any launch) and one bad argument at a time
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(buf)
    ptr += -ptr % 16
    good = dict(res=0.1, margin=64, B=1, H=256, W=256)

    def call(missing=None, grid=ptr, scratch=ptr, **kw):
        v = dict(good, **kw)
        ptrs = [ptr, grid, ptr, ptr, ptr, scratch, ptr, ptr]
        if missing is not None:
            ptrs[missing] = None
        return lib.pof_grid_scroll(ptrs[0], v["res"], v["margin"], v["B"], v["H"], v["W"], *ptrs[1:], None)

    for missing in range(8):
        assert call(missing=missing) == _lib.POF_E_BADARG, missing
    for bad in (dict(res=0.0), dict(res=-0.1), dict(res=float("nan")), dict(margin=-1), dict(margin=65),
                dict(margin=128), dict(margin=64, H=128), dict(margin=64, W=128), dict(margin=1, H=64, W=64),
                dict(margin=193, H=512, W=512), dict(B=-1)):
        assert call(**bad) == _lib.POF_E_BADARG, bad
    for bad in (dict(H=96), dict(W=96), dict(W=32), dict(H=2112), dict(W=100, margin=0), dict(grid=ptr + 8),
                dict(scratch=ptr + 2)):
        assert call(**bad) == _lib.POF_E_SHAPE, bad
    for fine in (dict(B=0), dict(B=0, margin=0), dict(B=0, margin=192, H=512, W=512), dict(B=0, margin=0, H=64, W=2048)):
        assert call(**fine) == _lib.POF_OK, fine
