"""The tile store behind the scrolling grid (pof_grid_scroll_store, N20) without a GPU: ``grid_scroll_store_oracle`` is
the NumPy restatement of the comment in include/pof_abi.h, built on ``grid_scroll_oracle`` (N14, tests/test_grid_scroll.py)
so that everything N14 writes is N14's.  It is checked here on rule scenes with exact numbers (res = 0.125, grids in
which every cell holds a value of its own, literal keys, stamps, counts and cells, and a literal Python loop over the
tiles), against N14 where nothing returns, and on ray-cast drives out and back for what the stage is for: the window
and its store together hold the cells a fixed map of the whole site holds, with no tolerance.
tests/test_grid_store_gpu.py imports the restatement and the scenes and holds the device to them bit for bit.

The stage adds integers and bitwise copies to N14: there is no ambiguous scene and no tolerance."""
import inspect
import os
import re

import numpy as np
import pytest

from test_grid_map import DEFAULTS as MAP_DEFAULTS, grid_map_oracle
from test_grid_match import CELL, DEFAULTS as MATCH_DEFAULTS, grid_match_oracle, pose_terms
from test_grid_refine import grid_refine_oracle
from test_grid_scroll import (CAP_OFFSET, RES, TILE, _sensor, axis_shift, default_margin, grid_scroll_oracle, numbered,
                              rule_scenes as scroll_scenes, step_trans, straight_drive)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_SLOTS = 1024
MUTATIONS = ("descending", "key_after", "no_reuse", "store_empty", "stamp_clock")


# ---------------------------------------------------------------- restatement of the device rule, one sensor
def empty_store(S):
    """A reset store of S slots: all zeros."""
    return dict(tiles=np.zeros((S, TILE, TILE), np.int16), key=np.zeros((S, 2), np.int32), stamp=np.zeros(S, np.int32),
                clock=np.zeros(1, np.int32))


def copy_store(store):
    return {k: v.copy() for k, v in store.items()}


def tile_of(grid, tx, ty):
    """The view of tile (tx, ty) of a grid."""
    return grid[TILE * ty:TILE * (ty + 1), TILE * tx:TILE * (tx + 1)]


def grid_scroll_store_oracle(trans, grid, origin, base, offset, store, res, margin=None, mutate=()):
    """One call for one sensor.  trans, grid, origin, base, offset, res and margin are ``grid_scroll_oracle``'s, and that
    function is what moves them; ``store`` (``empty_store``) is UPDATED IN PLACE and keeps every bit without a shift.
    ``mutate``: names of MUTATIONS, rules turned round.
    -> dict(shift [2] int32, scrolled uint8, counts [4] int32 = (restored, stored, evicted, dropped))."""
    H, W = grid.shape
    TH, TW, S = H // TILE, W // TILE, len(store["stamp"])
    before, o = grid.copy(), offset.astype(np.int64)
    out = grid_scroll_oracle(trans, grid, origin, base, offset, res, margin)           # N14, word for word
    counts = np.zeros(4, np.int32)
    sx, sy = (int(v) for v in out["shift"])
    if not (sx or sy):
        return dict(out, counts=counts)
    o2 = o + (sx, sy)
    inside = lambda x, y: 0 <= x < TW and 0 <= y < TH
    # arriving tiles: looked up under the offset behind the call, in the stamps as the call found them
    effective = store["stamp"].copy()
    held = {}                                                  # world tile -> the lowest occupied slot that holds it
    for j in np.flatnonzero(store["stamp"]):
        held.setdefault(tuple(int(v) for v in store["key"][j]), int(j))
    for ty in range(TH):
        for tx in range(TW):
            if inside(tx + sx, ty + sy):
                continue
            j = held.get((int(o2[0]) + tx, int(o2[1]) + ty))
            if j is not None:
                tile_of(grid, tx, ty)[...] = store["tiles"][j]
                effective[j] = 0                               # released
                counts[0] += 1
    # departing tiles that hold something, in ascending tile index, under the offset in front of the call
    ranked = []
    for ty in range(TH):
        for tx in range(TW):
            cells = tile_of(before, tx, ty)
            if not inside(tx - sx, ty - sy) and (cells.any() or "store_empty" in mutate):
                ranked.append(((o2 if "key_after" in mutate else o) + (tx, ty), cells))
    if "descending" in mutate:
        ranked.reverse()
    order = sorted(range(S), key=lambda j: ((store["stamp"] if "no_reuse" in mutate else effective)[j], j))
    stamp = effective.copy()                                   # a released slot that nothing takes ends free
    now = int(store["clock"][0]) + 1
    for r, (k, cells) in enumerate(ranked):
        if r >= S:
            counts[3] += 1
            continue
        j = order[r]
        store["tiles"][j] = cells
        store["key"][j] = k
        stamp[j] = now - 1 if "stamp_clock" in mutate else now
        counts[1] += 1
        counts[2] += int(effective[j] != 0)
    store["stamp"][...] = stamp
    store["clock"][0] = now
    return dict(out, counts=counts)


def literal_store_call(shift, grid, offset, store):
    """The rule as the header words it, one Python loop per tile, slot and rank and no helper of the restatement: the
    grid, the store and the counts behind a call whose shift is given (not 0) -> (grid', store', counts).  For the rule
    scenes only."""
    sx, sy = shift
    H, W = grid.shape
    TH, TW, S = H // TILE, W // TILE, len(store["stamp"])
    new, st = np.zeros_like(grid), copy_store(store)
    released = [False] * S
    restored = stored = evicted = dropped = 0
    for ty in range(TH):
        for tx in range(TW):
            ux, uy = tx + sx, ty + sy
            if 0 <= ux < TW and 0 <= uy < TH:                  # a tile that stays inside moves
                for y in range(TILE):
                    new[TILE * ty + y, TILE * tx:TILE * tx + TILE] = grid[TILE * uy + y, TILE * ux:TILE * ux + TILE]
                continue
            kx, ky = int(offset[0]) + sx + tx, int(offset[1]) + sy + ty
            for j in range(S):
                if store["stamp"][j] != 0 and store["key"][j][0] == kx and store["key"][j][1] == ky:
                    new[TILE * ty:TILE * ty + TILE, TILE * tx:TILE * tx + TILE] = store["tiles"][j]
                    released[j] = True
                    restored += 1
                    break
    taken = [False] * S
    for index in range(TH * TW):                               # ascending tile index
        tx, ty = index % TW, index // TW
        vx, vy = tx - sx, ty - sy
        if 0 <= vx < TW and 0 <= vy < TH:
            continue
        cells = grid[TILE * ty:TILE * ty + TILE, TILE * tx:TILE * tx + TILE]
        if not any(int(c) != 0 for c in cells.ravel()):
            continue
        # the first slot of the order that nobody took: the smallest effective stamp, then the lowest index
        best = None
        for j in range(S):
            if taken[j]:
                continue
            e = 0 if released[j] else int(store["stamp"][j])
            if best is None or e < best[0]:
                best = (e, j)
        if best is None:
            dropped += 1
            continue
        e, j = best
        taken[j] = True
        st["tiles"][j] = cells
        st["key"][j] = (int(offset[0]) + tx, int(offset[1]) + ty)
        st["stamp"][j] = int(store["clock"][0]) + 1
        stored += 1
        evicted += int(e != 0)
    for j in range(S):
        if released[j] and not taken[j]:
            st["stamp"][j] = 0
    st["clock"][0] = int(store["clock"][0]) + 1
    return new, st, np.array([restored, stored, evicted, dropped], np.int32)


# ---------------------------------------------------------------- rule scenes: exact numbers
def seeded_store(S, stamps, keys, clock, seed=7):
    """A store as earlier calls may have left it: the given stamps and keys, tiles of small random cells."""
    st = empty_store(S)
    st["tiles"][...] = np.random.default_rng(seed).integers(1, 90, (S, TILE, TILE)).astype(np.int16)
    st["stamp"][...] = stamps
    st["key"][...] = keys
    st["clock"][0] = clock
    return st


def _stored(sensor, store):
    return dict(sensor, store=store)


def _scene(H, W, margin, S, *sensors, res=RES):
    return dict(H=H, W=W, margin=margin, S=S, res=res, sensors=list(sensors))


def _with_grid(sensor, grid):
    return dict(sensor, grid=grid)


def sparse_grid():
    """128 x 128: tile (0, 0) all zeros, tile (0, 1) one cell, its last, the right half numbered."""
    g = numbered(128, 128, 3)
    g[:, :64] = 0
    g[127, 63] = -5
    return g


RIGHT, BACK, FULL = (128, 70), (-1, 70), (192, 70)             # 128 x 128, margin 0: shifts (1, 0), (-2, 0), (2, 0)
FAR = [(100 + j, 100) for j in range(4)]                       # keys no scene's window reaches


def rule_scenes():
    """-> {name: scene}; a scene is dict(H, W, margin, S, res, sensors=[dict(grid, origin, base, offset, steps and,
    where a store is given, store)]).  ``EXPECTED`` holds the shifts and counts, the tests below the keys, stamps and
    cells."""
    scenes = {
        # 128 x 128 has 2 x 2 tiles and takes margin 0: beyond the high border the shift is +1, beyond the low one -2
        "128 right and back": _scene(128, 128, 0, 16, _sensor(128, 128, [RIGHT, BACK])),
        "128 diagonal": _scene(128, 128, 0, 16, _sensor(128, 128, [(128, 128), (-1, -1)])),
        "128 full size": _scene(128, 128, 0, 16, _sensor(128, 128, [FULL])),
        # TH = 3, TW = 4, margin 64: y alone, one tile up and one tile back
        "192x256 y only": _scene(192, 256, 64, 16, _sensor(192, 256, [(130, 128), (130, 63)])),
        "128 sparse": _scene(128, 128, 0, 16, _with_grid(_sensor(128, 128, [RIGHT]), sparse_grid())),
        # the eviction order: slot 2 is free, slots 1 and 3 are the oldest, slot 0 the youngest
        "128 eviction, four leave": _scene(128, 128, 0, 4, _stored(_sensor(128, 128, [FULL]),
                                                                   seeded_store(4, [5, 3, 0, 3], FAR, 7))),
        "128 eviction, two leave": _scene(128, 128, 0, 4, _stored(_sensor(128, 128, [RIGHT]),
                                                                  seeded_store(4, [5, 3, 0, 3], FAR, 7))),
        # slots 1 and 2 hold the tiles that come back: released, they go first, in front of the older slot 0
        "128 released and reused": _scene(128, 128, 0, 3, _stored(_sensor(128, 128, [BACK]), seeded_store(
            3, [2, 3, 4], [(9, 9), (-1, 0), (-1, 1)], 4))),
        # one slot: world tile (0, 0) is stored, then evicted by (1, 0); back over both, (0, 0) is unknown
        "128 evicted before it returns": _scene(128, 128, 0, 1, _sensor(128, 128, [RIGHT, RIGHT, BACK])),
        # keys at the offset cap: 256 x 256, margin 64, the column tx = 0 leaves
        "256 keys at the cap": _scene(256, 256, 64, 16, _sensor(256, 256, [(192, 140)],
                                                                offset=(CAP_OFFSET - 1, 1 - CAP_OFFSET), seed=4)),
    }
    for S in (1, 2, 3):
        scenes["128 four leave, %d slots" % S] = _scene(128, 128, 0, S, _sensor(128, 128, [FULL], seed=S))
    # N14's scenes of spoiled positions, caps and a mixed batch, every sensor with a store that holds something
    for name in ("256 spoiled", "256 cap", "128x192 mixed"):
        s = scroll_scenes()[name]
        scenes[name] = _scene(s["H"], s["W"], s["margin"], 4, *[_stored(sensor, seeded_store(
            4, [2, 0, 1, 3], FAR, 3, seed=10 + b)) for b, sensor in enumerate(s["sensors"])])
    return scenes


# what every call of every sensor of a scene must answer: (shift, counts = (restored, stored, evicted, dropped))
Z = (0, 0, 0, 0)
EXPECTED = {
    "128 right and back": [[((1, 0), (0, 2, 0, 0)), ((-2, 0), (2, 2, 0, 0))]],
    "128 diagonal": [[((1, 1), (0, 3, 0, 0)), ((-2, -2), (1, 1, 0, 0))]],
    "128 full size": [[((2, 0), (0, 4, 0, 0))]],
    "192x256 y only": [[((0, 1), (0, 4, 0, 0)), ((0, -1), (4, 0, 0, 0))]],
    "128 sparse": [[((1, 0), (0, 1, 0, 0))]],
    "128 eviction, four leave": [[((2, 0), (0, 4, 3, 0))]],
    "128 eviction, two leave": [[((1, 0), (0, 2, 1, 0))]],
    "128 released and reused": [[((-2, 0), (2, 3, 1, 1))]],
    "128 evicted before it returns": [[((1, 0), (0, 1, 0, 1)), ((1, 0), (0, 1, 1, 1)), ((-2, 0), (1, 0, 0, 0))]],
    "256 keys at the cap": [[((1, 0), (0, 4, 0, 0))]],
    "128 four leave, 1 slots": [[((2, 0), (0, 1, 0, 3))]],
    "128 four leave, 2 slots": [[((2, 0), (0, 2, 0, 2))]],
    "128 four leave, 3 slots": [[((2, 0), (0, 3, 0, 1))]],
    "256 spoiled": [[((0, 0), Z)]] * 6,
    # a shift of 2^20 tiles empties the window: 16 tiles leave for 4 slots, of which one is free
    "256 cap": [[((CAP_OFFSET, 0), (0, 4, 3, 12)), ((0, 0), Z)], [((0, 0), Z), ((0, 1), (0, 4, 3, 0))],
                [((0, -CAP_OFFSET), (0, 4, 3, 12)), ((0, 0), Z)], [((0, 1), (0, 4, 3, 0)), ((0, 0), Z)],
                [((1, 0), (0, 4, 3, 0)), ((-2, 0), (4, 4, 0, 0))]],
    "128x192 mixed": [[((0, 0), Z), ((0, 0), Z)], [((0, 0), Z), ((2, 0), (0, 4, 3, 0))], [((0, 0), Z), ((0, 0), Z)],
                      [((0, 0), Z), ((2, 1), (0, 4, 3, 1))]],
}


def run_scene(scene, mutate=()):
    """The restatement over every sensor of a scene -> per sensor a list with one dict per call: trans (the input),
    shift, scrolled, counts, and copies of grid, origin, offset and the four store fields behind the call."""
    out = []
    for s in scene["sensors"]:
        grid, origin, offset = s["grid"].copy(), s["origin"].copy(), s["offset"].copy()
        store = copy_store(s["store"]) if "store" in s else empty_store(scene["S"])
        calls = []
        for step in s["steps"]:
            trans = step_trans(s, step, origin, scene["res"])
            o = grid_scroll_store_oracle(trans, grid, origin, s["base"], offset, store, scene["res"], scene["margin"], mutate)
            calls.append(dict(o, trans=trans, grid=grid.copy(), origin=origin.copy(), offset=offset.copy(),
                              **copy_store(store)))
        out.append(calls)
    return out


@pytest.fixture(scope="module")
def rules():
    return {k: run_scene(s) for k, s in rule_scenes().items()}


def test_every_scene_has_its_expected_shifts_and_counts(rules):
    assert set(EXPECTED) == set(rules)
    for name, sensors in rules.items():
        got = [[(tuple(int(v) for v in c["shift"]), tuple(int(v) for v in c["counts"])) for c in calls] for calls in sensors]
        assert got == [list(e) for e in EXPECTED[name]], (name, got)
        for calls in sensors:
            for c in calls:
                assert c["counts"].dtype == np.int32 and c["scrolled"] == (1 if c["shift"].any() else 0)


def test_every_rule_scene_equals_the_literal_loop(rules):
    for name, scene in rule_scenes().items():
        for s, calls in zip(scene["sensors"], rules[name]):
            grid, offset = s["grid"], s["offset"]
            store = s["store"] if "store" in s else empty_store(scene["S"])
            for c in calls:
                shift = tuple(int(v) for v in c["shift"])
                if shift == (0, 0):
                    want = (grid, store, np.zeros(4, np.int32))
                else:
                    want = literal_store_call(shift, grid, offset, store)
                assert np.array_equal(c["grid"], want[0]), name
                for f in ("tiles", "key", "stamp", "clock"):
                    assert np.array_equal(c[f], want[1][f]), (name, f)
                assert np.array_equal(c["counts"], want[2]), name
                grid, offset, store = c["grid"], c["offset"], {f: c[f] for f in ("tiles", "key", "stamp", "clock")}


def test_one_tile_to_the_right_and_back(rules):
    """A 2 x 2 grid with margin 0 goes +1 tile beyond its high border and -2 beyond its low one, so `back` is a shift of
    the grid's size: all four tiles arrive, world tiles (0, 0) and (0, 1) from slots 0 and 1, which are released -- and
    taken again at once by the two tiles that leave and hold something, the rule of the slot order."""
    g0 = rule_scenes()["128 right and back"]["sensors"][0]["grid"]
    away, back = rules["128 right and back"][0]
    assert away["key"][:2].tolist() == [[0, 0], [0, 1]] and away["stamp"].tolist() == [1, 1] + [0] * 14
    assert away["clock"].tolist() == [1] and away["offset"].tolist() == [1, 0]
    assert np.array_equal(away["tiles"][0], g0[:64, :64]) and np.array_equal(away["tiles"][1], g0[64:, :64])
    assert np.array_equal(away["grid"][:, :64], g0[:, 64:]) and not away["grid"][:, 64:].any()
    # back: the window is world x in {-1, 0}; the two tiles are back bit for bit, beside a column nobody has seen
    assert back["offset"].tolist() == [-1, 0] and back["clock"].tolist() == [2]
    assert np.array_equal(back["grid"][:, 64:], g0[:, :64]) and not back["grid"][:, :64].any()
    # what left is world x = 1, the old right half (x = 2 is unknown and takes no slot)
    assert back["key"][:2].tolist() == [[1, 0], [1, 1]] and back["stamp"].tolist() == [2, 2] + [0] * 14
    assert np.array_equal(back["tiles"][0], g0[:64, 64:]) and np.array_equal(back["tiles"][1], g0[64:, 64:])


def test_a_diagonal_and_a_full_size_shift(rules):
    g0 = rule_scenes()["128 diagonal"]["sensors"][0]["grid"]
    away, back = rules["128 diagonal"][0]
    assert away["key"][:3].tolist() == [[0, 0], [1, 0], [0, 1]] and away["stamp"][:4].tolist() == [1, 1, 1, 0]
    assert np.array_equal(away["grid"][:64, :64], g0[64:, 64:]) and not away["grid"][64:].any() and not away["grid"][:, 64:].any()
    assert np.array_equal(away["tiles"][1], g0[:64, 64:]) and np.array_equal(away["tiles"][2], g0[64:, :64])
    # back by (-2, -2): world tile (0, 0) returns from slot 0, which the one tile that leaves, (1, 1), takes again
    assert back["offset"].tolist() == [-1, -1] and np.array_equal(back["grid"][64:, 64:], g0[:64, :64])
    assert not back["grid"][:64].any() and not back["grid"][:, :64].any()
    assert back["key"][:3].tolist() == [[1, 1], [1, 0], [0, 1]] and back["stamp"][:4].tolist() == [2, 1, 1, 0]
    assert np.array_equal(back["tiles"][0], g0[64:, 64:])
    g0 = rule_scenes()["128 full size"]["sensors"][0]["grid"]
    full = rules["128 full size"][0][0]
    assert not full["grid"].any() and full["key"][:4].tolist() == [[0, 0], [1, 0], [0, 1], [1, 1]]
    assert full["stamp"].tolist() == [1] * 4 + [0] * 12
    for j, (tx, ty) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        assert np.array_equal(full["tiles"][j], tile_of(g0, tx, ty))


def test_a_shift_on_y_only_with_unequal_tile_counts(rules):
    g0 = rule_scenes()["192x256 y only"]["sensors"][0]["grid"]
    up, back = rules["192x256 y only"][0]
    assert up["key"][:4].tolist() == [[0, 0], [1, 0], [2, 0], [3, 0]] and up["stamp"].tolist() == [1] * 4 + [0] * 12
    assert np.array_equal(up["grid"][:128], g0[64:]) and not up["grid"][128:].any()
    # back: the row comes back, the row that leaves is unknown, and the grid has every bit it started with
    assert back["grid"].tobytes() == g0.tobytes() and not back["stamp"].any() and back["clock"].tolist() == [2]
    assert back["offset"].tolist() == [0, 0] and back["origin"].tobytes() == rule_scenes()["192x256 y only"]["sensors"][0]["origin"].tobytes()


def test_an_empty_tile_takes_no_slot_and_one_cell_does(rules):
    g0 = rule_scenes()["128 sparse"]["sensors"][0]["grid"]
    assert not g0[:64, :64].any() and np.count_nonzero(g0[64:, :64]) == 1 and g0[127, 63] != 0
    c = rules["128 sparse"][0][0]
    assert c["key"][0].tolist() == [0, 1] and c["stamp"].tolist() == [1] + [0] * 15
    assert np.array_equal(c["tiles"][0], g0[64:, :64]) and not c["tiles"][1:].any()


def test_ranks_beyond_the_slots_are_dropped_in_tile_order(rules):
    keys = [[0, 0], [1, 0], [0, 1], [1, 1]]
    for S in (1, 2, 3):
        name = "128 four leave, %d slots" % S
        g0, c = rule_scenes()[name]["sensors"][0]["grid"], rules[name][0][0]
        assert c["key"].tolist() == keys[:S] and c["stamp"].tolist() == [1] * S
        for j in range(S):
            assert np.array_equal(c["tiles"][j], tile_of(g0, *keys[j]))


def test_eviction_takes_free_slots_then_the_smallest_stamp_then_the_lowest_index(rules):
    scene = rule_scenes()["128 eviction, four leave"]
    g0, c = scene["sensors"][0]["grid"], rules["128 eviction, four leave"][0][0]
    # stamps (5, 3, 0, 3): the order is slot 2, 1, 3, 0 for the tiles (0, 0), (1, 0), (0, 1), (1, 1)
    assert c["key"].tolist() == [[1, 1], [1, 0], [0, 0], [0, 1]] and c["stamp"].tolist() == [8] * 4 and c["clock"].tolist() == [8]
    assert np.array_equal(c["tiles"][2], g0[:64, :64]) and np.array_equal(c["tiles"][0], g0[64:, 64:])
    scene = rule_scenes()["128 eviction, two leave"]
    s, c = scene["sensors"][0], rules["128 eviction, two leave"][0][0]
    # tiles (0, 0) and (0, 1) leave: the free slot 2, then slot 1 in front of slot 3 of the same stamp
    assert c["key"].tolist() == [[100, 100], [0, 1], [0, 0], [103, 100]] and c["stamp"].tolist() == [5, 8, 8, 3]
    assert np.array_equal(c["tiles"][0], s["store"]["tiles"][0]) and np.array_equal(c["tiles"][3], s["store"]["tiles"][3])


def test_a_slot_released_in_a_call_is_reused_by_it_ahead_of_older_ones(rules):
    s = rule_scenes()["128 released and reused"]["sensors"][0]
    c = rules["128 released and reused"][0][0]
    # the tiles of slots 1 and 2 are back in the window, column tx = 1
    assert np.array_equal(c["grid"][:64, 64:], s["store"]["tiles"][1]) and np.array_equal(c["grid"][64:, 64:], s["store"]["tiles"][2])
    assert not c["grid"][:, :64].any()
    # slots 1, 2 (released), then 0 (stamp 2, evicted) take the tiles (0, 0), (1, 0), (0, 1); (1, 1) is dropped
    assert c["key"].tolist() == [[0, 1], [0, 0], [1, 0]] and c["stamp"].tolist() == [5, 5, 5] and c["clock"].tolist() == [5]
    assert np.array_equal(c["tiles"][1], s["grid"][:64, :64]) and np.array_equal(c["tiles"][0], s["grid"][64:, :64])


def test_a_tile_evicted_before_it_returns_comes_back_unknown(rules):
    g0 = rule_scenes()["128 evicted before it returns"]["sensors"][0]["grid"]
    a, b, c = rules["128 evicted before it returns"][0]
    assert a["key"].tolist() == [[0, 0]] and b["key"].tolist() == [[1, 0]] and b["stamp"].tolist() == [2]
    # the window is world x in {0, 1} again: (1, 0) is back, (0, 0) was evicted, the row y = 1 was dropped
    assert c["offset"].tolist() == [0, 0] and np.array_equal(c["grid"][:64, 64:], g0[:64, 64:])
    assert not c["grid"][:, :64].any() and not c["grid"][64:].any() and c["stamp"].tolist() == [0] and c["clock"].tolist() == [3]


def test_spoiled_positions_and_the_caps_store_nothing(rules):
    for name in ("256 spoiled", "256 cap"):
        for s, calls in zip(rule_scenes()[name]["sensors"], rules[name]):
            last = dict(s["store"], grid=s["grid"])
            for c in calls:
                if not c["shift"].any():
                    assert not c["counts"].any() and not c["scrolled"]
                    for f in ("tiles", "key", "stamp", "clock", "grid"):
                        assert c[f].tobytes() == last[f].tobytes(), (name, f)
                last = c
    assert all(not calls[0]["shift"].any() for calls in rules["256 spoiled"])


def test_a_mixed_batch_keeps_every_bit_of_the_sensors_that_stay(rules):
    for b, (s, calls) in enumerate(zip(rule_scenes()["128x192 mixed"]["sensors"], rules["128x192 mixed"])):
        last = calls[-1]
        if b in (0, 2):
            assert last["grid"].tobytes() == s["grid"].tobytes() and last["origin"].tobytes() == s["origin"].tobytes()
            for f in ("tiles", "key", "stamp", "clock"):
                assert last[f].tobytes() == s["store"][f].tobytes(), (b, f)
        else:
            assert last["scrolled"] and last["clock"].tolist() == [4] and (last["stamp"] == 4).sum() == 4


def test_keys_at_the_offset_cap(rules):
    c = rules["256 keys at the cap"][0][0]
    assert c["offset"].tolist() == [CAP_OFFSET, 1 - CAP_OFFSET]
    assert c["key"][:4].tolist() == [[CAP_OFFSET - 1, 1 - CAP_OFFSET + ty] for ty in range(4)] and c["key"].dtype == np.int32


def test_each_rule_turned_round_changes_a_named_scene(rules):
    named = {"descending": "128 four leave, 1 slots", "key_after": "128 right and back",
             "no_reuse": "128 released and reused", "store_empty": "128 sparse", "stamp_clock": "128 right and back"}
    assert set(named) == set(MUTATIONS)
    for mutation, name in named.items():
        got = run_scene(rule_scenes()[name], (mutation,))[0][-1]
        want = rules[name][0][-1]
        assert any(not np.array_equal(got[f], want[f]) for f in ("grid", "tiles", "key", "stamp", "counts")), mutation


def device_scenes():
    """-> {name: scene}: what tests/test_grid_store_gpu.py runs beside the rule scenes -- one sensor in 2048 x 2048 with a
    shift of the grid's size, so all 1024 tiles leave, for a store of 1024 and of 1023 slots whose stamps (a third of
    them free, the others 1-5) make the slot order a permutation of its own."""
    def big(S, seed):
        rng = np.random.default_rng(seed)
        s = _sensor(64, 64, [(1024 + 2048, 1024 - 2048)], origin=(-128.0, -128.0))
        s["grid"] = rng.integers(-40, 71, (2048, 2048)).astype(np.int16)
        stamps = rng.integers(0, 6, S) * (rng.random(S) > 0.33)
        return _stored(s, seeded_store(S, stamps, [(5000 + j, 7) for j in range(S)], 5, seed=seed))
    return {"2048 all leave, %d slots" % S: _scene(2048, 2048, 512, S, big(S, S)) for S in (MAX_SLOTS, MAX_SLOTS - 1)}


def test_device_scenes_reach_their_shapes():
    for name, scene in device_scenes().items():
        S, s = scene["S"], scene["sensors"][0]
        c = run_scene(scene)[0][0]
        occupied = int((s["store"]["stamp"] != 0).sum())
        assert c["shift"].tolist() == [32, -32] and not c["grid"].any() and 300 < occupied < 900
        # every slot is taken, so every occupied one is evicted
        assert c["counts"].tolist() == [0, S, occupied, MAX_SLOTS - S] and (c["stamp"] == 6).all(), name
        # rank order against slot order: the r-th tile lies in the r-th slot of (stamp, index)
        order = sorted(range(S), key=lambda j: (int(s["store"]["stamp"][j]), j))
        for r in (0, 1, 2, S // 2, S - 1):
            assert c["key"][order[r]].tolist() == [r % 32, r // 32]
            assert np.array_equal(c["tiles"][order[r]], tile_of(s["grid"], r % 32, r // 32)), (name, r)


# ---------------------------------------------------------------- equal to N14 where nothing returns
@pytest.mark.parametrize("seed", [21, 22, 31])
def test_a_drive_one_way_is_n14_bit_for_bit(seed):
    tab, scans, poses = straight_drive(seed, 27.0, 1.0, stretch=4.5)
    kw = dict(MAP_DEFAULTS, max_range=5.0)
    base = np.floor(poses[0, :2] / RES) * RES - 0.5 * RES * 256
    a = dict(grid=np.zeros((256, 256), np.int16), origin=base.copy(), offset=np.zeros(2, np.int32))
    b = dict(grid=np.zeros((256, 256), np.int16), origin=base.copy(), offset=np.zeros(2, np.int32))
    store, scrolls, restored = empty_store(64), 0, 0
    for scan, pose in zip(scans, poses):
        rot, trans = pose_terms(pose)
        want = grid_scroll_oracle(trans, a["grid"], a["origin"], base, a["offset"], RES, 64)
        got = grid_scroll_store_oracle(trans, b["grid"], b["origin"], base, b["offset"], store, RES, 64)
        scrolls += int(got["scrolled"])
        restored += int(got["counts"][0])
        assert np.array_equal(got["shift"], want["shift"]) and got["scrolled"] == want["scrolled"]
        for f in ("grid", "origin", "offset"):
            assert a[f].tobytes() == b[f].tobytes(), f
        for g in (a, b):
            grid_map_oracle(scan, tab, rot, trans, g["grid"], g["origin"], RES, **kw)
    assert scrolls >= 3 and restored == 0 and (store["stamp"] != 0).any()


# ---------------------------------------------------------------- the window and its store are the fixed map
WINDOW, WORLD, SLOTS, WINDOW_RANGE, WINDOW_MARGIN = 256, 1024, 64, 5.0, 64
WORLD_TILE = (2, 6)                                            # where the window's world tile (0, 0) lies in the map
OUT_AND_BACK_SEEDS = (21, 22)


def out_and_back(seed, length, step, **kw):
    """``straight_drive`` out along the lane and back over the same poses in reverse order (with the scans taken
    there) -> (tab, scans, poses, the number of scans of the way out)."""
    tab, scans, poses = straight_drive(seed, length, step, **kw)
    return tab, np.concatenate([scans, scans[::-1]]), np.concatenate([poses, poses[::-1]]), len(scans)


def window_store_and_map(seed):
    """A 256 x 256 window with its store, the same window with N14 alone, and a fixed 1024 x 1024 map of the same cells,
    driven with the same scans at the same poses, the scroll in front of the update.  Every condition and every
    equality is asserted after every scan; -> (scrolls out, scrolls back, cells of the N14 window that differ from the
    map on the way back, summed over its scans)."""
    tab, scans, poses, T_out = out_and_back(seed, 51.0, 1.5, stretch=10.5)
    kw = dict(MAP_DEFAULTS, max_range=WINDOW_RANGE)
    assert WINDOW_RANGE + RES < TILE * RES                     # a scan touches no cell a tile away from its sensor
    base = np.floor(poses[0, :2] / RES) * RES - 0.5 * RES * WINDOW
    world_origin = base - RES * TILE * np.array(WORLD_TILE, np.float64)
    win, origin, offset, store = np.zeros((WINDOW, WINDOW), np.int16), base.copy(), np.zeros(2, np.int32), empty_store(SLOTS)
    plain, p_origin, p_offset = win.copy(), base.copy(), offset.copy()
    world = np.zeros((WORLD, WORLD), np.int16)
    scrolls, differ = [0, 0], 0
    for t, (scan, pose) in enumerate(zip(scans, poses)):
        rot, trans = pose_terms(pose)
        o = grid_scroll_store_oracle(trans, win, origin, base, offset, store, RES, WINDOW_MARGIN)
        grid_scroll_oracle(trans, plain, p_origin, base, p_offset, RES, WINDOW_MARGIN)
        assert np.array_equal(offset, p_offset)
        assert o["counts"][2] == 0 and o["counts"][3] == 0, (seed, t)
        scrolls[t >= T_out] += int(o["scrolled"])
        cell = np.floor((trans - origin) / RES)
        assert ((cell >= WINDOW_MARGIN) & (cell < WINDOW - WINDOW_MARGIN)).all(), (seed, t, cell)
        grid_map_oracle(scan, tab, rot, trans, win, origin, RES, **kw)
        grid_map_oracle(scan, tab, rot, trans, plain, p_origin, RES, **kw)
        grid_map_oracle(scan, tab, rot, trans, world, world_origin, RES, **kw)
        tx0, ty0 = int(offset[0]) + WORLD_TILE[0], int(offset[1]) + WORLD_TILE[1]
        assert 0 <= tx0 <= (WORLD - WINDOW) // TILE and 0 <= ty0 <= (WORLD - WINDOW) // TILE
        part = world[TILE * ty0:TILE * ty0 + WINDOW, TILE * tx0:TILE * tx0 + WINDOW]
        assert np.array_equal(win, part), (seed, t, int((win != part).sum()))
        held = set()
        for j in np.flatnonzero(store["stamp"]):
            kx, ky = (int(v) for v in store["key"][j])
            held.add((kx, ky))
            assert np.array_equal(store["tiles"][j], tile_of(world, kx + WORLD_TILE[0], ky + WORLD_TILE[1])), (seed, t, j)
        assert len(held) == np.count_nonzero(store["stamp"])   # a world tile is in one slot
        for ty in range(WORLD // TILE):
            for tx in range(WORLD // TILE):
                in_window = tx0 <= tx < tx0 + WINDOW // TILE and ty0 <= ty < ty0 + WINDOW // TILE
                k = (tx - WORLD_TILE[0], ty - WORLD_TILE[1])
                assert not (in_window and k in held), (seed, t, k)             # in the window or in the store, not both
                if not in_window and tile_of(world, tx, ty).any():
                    assert k in held, (seed, t, k)
        if t >= T_out:
            differ += int((plain != part).sum())
    return scrolls[0], scrolls[1], differ


@pytest.mark.parametrize("seed", OUT_AND_BACK_SEEDS)
def test_the_window_and_its_store_are_the_fixed_map(seed):
    """51 m out along the lane of a long room and back, a scan every 1.5 m, 0.125 m cells, max_range 5 m: a 256 x 256
    window with margin 64 and a store of 64 tiles against a fixed 1024 x 1024 map.  After every scan every cell of the
    window equals the map's, every occupied slot equals the map's tile at its key, and every tile of the map outside
    the window that holds something is in the store; nothing is evicted or dropped.  A window of four tiles with margin
    64 goes out a tile at a time and comes back two at a time, so the drive is long enough for three scrolls back.
    Measured with this restatement, seeds 21 and 22: 6 scrolls out and 3 back in each, no cell differs; N14 alone
    differs from the map on the way back in 341139 / 223814 cells (summed over its 35 scans)."""
    out, back, differ = window_store_and_map(seed)
    print("seed %d: %d scrolls out, %d back; N14 alone differs from the map in %d cells over the way back"
          % (seed, out, back, differ))
    assert out >= 3 and back >= 3, seed
    assert differ >= 1, seed


CHAIN_SEED, CHAIN_SLOTS = 21, 16


def chain():
    """The chain tests/test_grid_store_gpu.py runs through ``ops.grid_scroll_store`` + ``ops.grid_map_update``: six scans
    6.5 m apart out along the lane and the same six back, a 256 x 256 window of 0.125 m cells with margin 64 and
    max_range 5 m.  -> (tab, scans, poses, base, per scan a dict of what the restatement leaves: rot, trans, shift,
    scrolled, counts, grid, origin, offset, the store's fields and the outputs of the map update)."""
    tab, scans, poses, _ = out_and_back(CHAIN_SEED, 32.5, 6.5, stretch=7.5)
    kw = dict(MAP_DEFAULTS, max_range=WINDOW_RANGE)
    base = np.floor(poses[0, :2] / RES) * RES - 0.5 * RES * WINDOW
    grid, origin, offset, store = np.zeros((WINDOW, WINDOW), np.int16), base.copy(), np.zeros(2, np.int32), empty_store(CHAIN_SLOTS)
    steps = []
    for scan, pose in zip(scans, poses):
        rot, trans = pose_terms(pose)
        o = grid_scroll_store_oracle(trans, grid, origin, base, offset, store, RES, WINDOW_MARGIN)
        m = grid_map_oracle(scan, tab, rot, trans, grid, origin, RES, **kw)
        steps.append(dict(o, rot=rot, trans=trans, grid=grid.copy(), origin=origin.copy(), offset=offset.copy(),
                          map=m, **copy_store(store)))
    return tab, scans, poses, base, steps


def test_the_chain_of_the_device_test_scrolls_twice_each_way_and_restores():
    from test_grid_map import ambiguous_cells
    tab, scans, poses, base, steps = chain()
    assert len(steps) == 12
    out = sum(int(s["scrolled"]) for s in steps[:6])
    back = sum(int(s["scrolled"]) for s in steps[6:])
    restored = sum(int(s["counts"][0]) for s in steps)
    print("chain: %d scrolls out, %d back, %d tiles restored, shifts %s" % (out, back, restored, [s["shift"].tolist() for s in steps]))
    assert out >= 2 and back >= 2 and restored >= 2
    assert all(s["counts"][2] == 0 and s["counts"][3] == 0 for s in steps)
    for s in steps:
        assert ambiguous_cells(tab, s["rot"], s["trans"], s["origin"], RES, WINDOW, WINDOW, WINDOW_RANGE) == 0


# ---------------------------------------------------------------- what the stage is good for
QUALITY_SEEDS = (31, 32, 33)
QUALITY_LENGTH, QUALITY_STEP = 31.25, 1.25


def _quality(seed):
    """The out-and-back drive at the defaults (0.1 m cells, 256 x 256, the default margin, max_range 20 m), once with
    the store and once with N14 alone, the scroll in front of the update.  On the scans of the way back -> per variant
    (endpoints inside the grid, the share of them on cells with a prior >= hit, the scans whose grid_match from the true
    pose is ok, those whose grid_refine is ok), and the scans of the way back."""
    tab, scans, poses, T_out = out_and_back(seed, QUALITY_LENGTH, QUALITY_STEP)
    out = {}
    for name in ("store", "n14"):
        base = poses[0, :2] - 0.5 * CELL * 256
        grid, origin, offset, store = np.zeros((256, 256), np.int16), base.copy(), np.zeros(2, np.int32), empty_store(64)
        seen = known = matched = refined = 0
        for t, (scan, pose) in enumerate(zip(scans, poses)):
            rot, trans = pose_terms(pose)
            if name == "store":
                grid_scroll_store_oracle(trans, grid, origin, base, offset, store, CELL)
            else:
                grid_scroll_oracle(trans, grid, origin, base, offset, CELL)
            if t >= T_out:
                matched += int(grid_match_oracle(scan, tab, rot, trans, pose, grid, origin, CELL, **MATCH_DEFAULTS)["ok"])
                refined += int(grid_refine_oracle(scan, tab, pose, grid, origin, CELL)["ok"])
            last = grid_map_oracle(scan, tab, rot, trans, grid, origin, CELL)
            if t >= T_out:
                inside = last["point_cell"] >= 0
                seen += int(inside.sum())
                known += int((last["point_prior"][inside] >= MAP_DEFAULTS["hit"]).sum())
        out[name] = (seen, known / max(seen, 1), matched, refined)
    return out, len(scans) - T_out


def test_quality_on_the_way_back():
    """Measured with this restatement (recorded in DESIGN.md 8, N20), seeds 31-33, 26 scans 1.25 m apart out and the
    same 26 back: of the return leg's endpoints inside the grid (10635 / 9407 / 9835, the same with and without) the
    share on cells with a prior >= hit is 0.995 / 0.999 / 0.999 with the store and 0.863 / 0.916 / 0.892 with N14 alone.
    From the true pose grid_match is ok at 26 / 26 / 26 of the 26 return scans with the store and at 25 / 26 / 25
    without, grid_refine at 24 / 26 / 26 either way: with 20 m of range much of every scan lands on the part of the
    window that never left, which is enough for both gates at a true pose -- what the store adds at these settings is
    the map under the rest.  Asserted: the share is strictly larger with the store in every seed; N14 alone is the
    yardstick."""
    for seed in QUALITY_SEEDS:
        q, T_back = _quality(seed)
        print("seed %d, %d return scans: endpoints inside / share known / grid_match ok / grid_refine ok: with the store "
              "%d / %.3f / %d / %d, N14 alone %d / %.3f / %d / %d" % ((seed, T_back) + q["store"] + q["n14"]))
        assert q["store"][0] > 0 and q["n14"][0] > 0, seed
        assert q["store"][1] > q["n14"][1], seed


# ---------------------------------------------------------------- surface
def test_records_and_settings_against_literal_tables():
    import torch
    from planar_optical_flow_amd import ops, streaming
    B, H, W, S = 2, 64, 128, 5                                 # pairwise distinct: a transposed shape cannot pass
    i32, i16, u8 = torch.int32, torch.int16, torch.uint8
    records = {
        "grid_store_state": ((B, H, W, S), "GridStoreState", (
            ("store", i16, (2, 5, 64, 64)), ("store_key", i32, (2, 5, 2)), ("store_stamp", i32, (2, 5)),
            ("clock", i32, (2,)), ("plan_in", i32, (2, 2)), ("plan_out", i32, (2, 2)))),
        "grid_scroll_store_buffers": ((B,), "GridScrollStore", (
            ("shift", i32, (2, 2)), ("scrolled", u8, (2,)), ("counts", i32, (2, 4)))),
    }
    for fn, (args, cls, fields) in records.items():
        rec = getattr(ops, fn)(*args, device="cpu")
        assert type(rec) is getattr(ops, cls) and type(rec).__name__ == cls, fn
        assert rec._fields == tuple(f for f, _, _ in fields), fn
        for (f, dtype, shape), t in zip(fields, rec):
            assert (t.dtype, tuple(t.shape), t.device.type) == (dtype, shape, "cpu"), (fn, f)
            assert not t.any(), (fn, f)
    assert ops.GridStoreState.persistent == ("store", "store_key", "store_stamp", "clock")
    assert ops.GridScrollStore.persistent == ()
    # N14's records and settings stay what they are
    assert ops.GridScrollState._fields == ("base", "offset", "scratch") and ops.GridScroll._fields == ("shift", "scrolled")
    assert ops.stage_settings(ops.grid_scroll_store) == ops.stage_settings(ops.grid_scroll) == dict(res=ops.REQUIRED, margin=None)
    assert streaming.stage_defaults("grid_scroll") == dict(margin=None)
    assert streaming.stage_defaults("grid_store") == {"slots": 64} == streaming.stage_settings("grid_store", {})
    assert streaming.stage_settings("grid_store", dict(slots=8)) == dict(slots=8)
    for unknown in ("margin", "res", "size", "no_such_setting"):
        with pytest.raises(ValueError, match="unknown grid_store settings"):
            streaming.stage_settings("grid_store", {unknown: 1})
    for bad in (0, -1, MAX_SLOTS + 1):
        with pytest.raises(ValueError):
            ops.grid_store_state(1, 64, 64, bad, device="cpu")
    for bad in ((96, 64), (64, 32), (2112, 64)):
        with pytest.raises(ValueError):
            ops.grid_store_state(1, bad[0], bad[1], 4, device="cpu")
    assert ops.grid_store_state(1, 2048, 2048, MAX_SLOTS, device="meta").plan_in.shape == (1, 1024)
    # grid_store_reset: stamps and clock <- 0 with tensor ops; the rest is dead without a stamp
    store = ops.grid_store_state(B, H, W, S, device="cpu")
    for t in store:
        t.fill_(7)
    assert ops.grid_store_reset(store) is not None
    assert not store.store_stamp.any() and not store.clock.any() and bool((store.store_key == 7).all())


def test_header_binding_and_wrappers():
    import torch
    from planar_optical_flow_amd import _lib, ops
    from planar_optical_flow_amd.src.utils import utils
    from planar_optical_flow_amd.streaming import StreamingDetector
    text = open(os.path.join(REPO, "include", "pof_abi.h")).read()
    m = re.search(r"\bint\s+pof_grid_scroll_store\s*\(([^)]*)\)\s*;", text)
    assert m, "include/pof_abi.h does not declare pof_grid_scroll_store"
    params = [p.strip() for p in m.group(1).split(",")]
    restype, argtypes = _lib.SIGNATURES["pof_grid_scroll_store"]
    assert restype is _lib._i and len(argtypes) == len(params) == 22
    for p, t in zip(params, argtypes):
        want = _lib._p if "*" in p or p.startswith("pof_stream_t") else _lib._d if p.startswith("double") else _lib._i
        assert t is want, p
    # the records are unpacked positionally into the call: state, scroll, store, out in the header's order
    names = [re.sub(r".*[ *]", "", p) for p in params]
    assert names[:7] == ["trans", "res", "margin", "slots", "B", "H", "W"]
    assert names[7:21] == list(ops.GridMapState._fields + ops.GridScrollState._fields + ops.GridStoreState._fields +
                               ops.GridScrollStore._fields)
    # N14's declaration stands as it was
    assert re.search(r"\bint\s+pof_grid_scroll\s*\(([^)]*)\)\s*;", text).group(1).count(",") == 13
    assert "N20" in text and "store_stamp" in text and "#define POF_ABI_VERSION 1" in text
    for name in ("grid_scroll_store", "grid_scroll_store_buffers", "grid_store_state", "grid_store_reset"):
        assert callable(getattr(ops, name))
    p = inspect.signature(ops.grid_scroll_store).parameters
    assert list(p) == ["trans", "state", "scroll", "store", "res", "margin", "out"]
    assert p["res"].kind is inspect.Parameter.KEYWORD_ONLY and p["res"].default is inspect.Parameter.empty
    assert p["margin"].default is None and p["out"].default is None
    assert list(inspect.signature(ops.grid_store_state).parameters) == ["B", "H", "W", "slots", "device"]
    assert inspect.signature(utils.OccupancyGrid.__init__).parameters["store"].default is None
    assert isinstance(utils.OccupancyGrid.store_tiles, property)
    assert inspect.signature(StreamingDetector.__init__).parameters["grid_store"].default is None
    assert callable(StreamingDetector.grid_store)
    # no CPU path
    f64 = torch.float64
    state = ops.grid_map_state(1, 64, 64, device="cpu")
    scroll = ops.grid_scroll_state(1, 64, 64, device="cpu")
    store = ops.grid_store_state(1, 64, 64, 4, device="cpu")
    with pytest.raises(TypeError):
        ops.grid_scroll_store(torch.zeros(1, 2, dtype=f64), state, scroll, store, res=0.1)
    with pytest.raises(TypeError):
        ops.grid_scroll_store(None, None, None, None, res=0.1)
    # the wrapper refuses wrong settings before it touches a device, and a store needs a scroll
    with pytest.raises(ValueError, match="give both"):
        utils.OccupancyGrid(np.zeros(4), store=dict(slots=8))
    for bad in (dict(slots=0), dict(slots=MAX_SLOTS + 1), dict(slot=8), dict(slots=8, margin=0)):
        with pytest.raises(ValueError):
            utils.OccupancyGrid(np.zeros(4), scroll=dict(), store=bad)


def test_entry_point_refuses_null_and_bad_arguments():
    import ctypes
    from planar_optical_flow_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "pof_grid_scroll_store")
    _, argtypes = _lib.SIGNATURES["pof_grid_scroll_store"]
    assert lib.pof_grid_scroll_store(*[None if t is _lib._p else 0 for t in argtypes]) == _lib.POF_E_BADARG
    assert lib.pof_grid_scroll_store(*[None if t is _lib._p else 1 for t in argtypes]) == _lib.POF_E_BADARG
    # every pointer given (never read: a refusal comes before any launch) and one bad argument at a time
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(buf)
    ptr += -ptr % 16
    good = dict(res=0.1, margin=64, slots=8, B=1, H=256, W=256)

    def call(missing=None, grid=ptr, scratch=ptr, store=ptr, **kw):
        v = dict(good, **kw)
        ptrs = [ptr, grid, ptr, ptr, ptr, scratch, store] + [ptr] * 8
        if missing is not None:
            ptrs[missing] = None
        return lib.pof_grid_scroll_store(ptrs[0], v["res"], v["margin"], v["slots"], v["B"], v["H"], v["W"], *ptrs[1:], None)

    for missing in range(15):
        assert call(missing=missing) == _lib.POF_E_BADARG, missing
    for bad in (dict(slots=0), dict(slots=-3), dict(slots=MAX_SLOTS + 1), dict(res=0.0), dict(res=float("nan")),
                dict(margin=-1), dict(margin=65), dict(margin=64, H=128), dict(B=-1), dict(slots=0, B=0)):
        assert call(**bad) == _lib.POF_E_BADARG, bad
    for bad in (dict(H=96), dict(W=32), dict(H=2112), dict(grid=ptr + 8), dict(scratch=ptr + 2), dict(store=ptr + 8),
                dict(store=ptr + 2, B=0)):
        assert call(**bad) == _lib.POF_E_SHAPE, bad
    for fine in (dict(B=0), dict(B=0, slots=1), dict(B=0, slots=MAX_SLOTS), dict(B=0, margin=0, H=64, W=2048)):
        assert call(**fine) == _lib.POF_OK, fine
