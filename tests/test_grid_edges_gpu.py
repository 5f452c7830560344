"""The occupancy-grid stages on the GPU where tiles, slices and limits decide: pof_grid_map_update and pof_grid_match
against the restatements of tests/test_grid_map.py and tests/test_grid_match.py, BIT FOR BIT, on the scenes of
tests/test_grid_edges.py (which asserts what each scene is built to reach: a tile exactly on the boundary of an early exit,
staged points on all four borders of a 2048-cell grid, every slice count, scores at +-4096 x 32767, ...).

The map runs from a prior grid that is not empty: the grid is uploaded, one scan is entered, and the grid and the five
outputs are compared (integers; tests/test_grid_edges.py asserts for every scene that no cell is within 1e-9 of the
boundary between two beams).  The match is compared as tests/test_grid_match_gpu.py does: scores, best, score, votes, ok,
moved, correction, pose and trans as bits; rot as the incoming bits without ``moved`` and to one float32 ulp with it."""
import numpy as np
import pytest
import torch

from test_grid_edges import (FREE_EDGES, G_SCENES, MAGNITUDES, NON_FINITE, PACK_SHAPES, equal_cases, extreme_cases,
                             far_and_small_cases, free_edge_scenes, general_scene, hit_edge_scenes, long_scan_cases,
                             packing_case, reach_cases, run_prior, small_table_scenes, spoiled_pose_scenes)
from test_grid_map import OUT_DTYPES as MAP_DTYPES
from test_grid_map_gpu import FIELDS as MAP_FIELDS, _host as map_host, _inputs as map_inputs, _state as map_state
from test_grid_match_gpu import check_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from planar_optical_flow_amd import ops as _ops
    return _ops


def check_prior_scene(ops, scene, what):
    """One scan of every sensor of the scene in one batch, from the sensors' prior grids: every field the restatement's."""
    sensors = scene["sensors"]
    N = len(sensors[0]["scans"][0]["ranges"])
    state, out = map_state(ops, scene, sensors), ops.grid_map_buffers(len(sensors), N)
    state.grid.copy_(torch.from_numpy(np.stack([s["prior"] for s in sensors])).cuda())
    args, nms = map_inputs([s["scans"][0] for s in sensors], scene["tab"])
    ops.grid_map_update(*args, state, res=scene["res"], out=out, **nms, **scene["kw"])
    got = map_host(out, state)
    changed = 0
    for b, sensor in enumerate(sensors):
        want = run_prior(scene, sensor)[0]
        for k, dt in zip(MAP_FIELDS, MAP_DTYPES + (np.int16,)):
            differ = int((got[k][b] != want[k]).sum())
            assert got[k].dtype == dt and differ == 0, (what, b, k, differ)
        changed += int((want["grid"] != sensor["prior"]).sum())
    return changed


# ------------------------------------------------------------------ A. the map
@pytest.fixture(scope="module")
def free_edges():
    return free_edge_scenes()


@pytest.mark.parametrize("which", ["at", "above"])
@pytest.mark.parametrize("name", sorted(FREE_EDGES))
def test_tile_at_the_boundary_of_can_free(ops, free_edges, name, which):
    scene = free_edges[(name, which)]
    changed = check_prior_scene(ops, scene, (name, which))
    (H, W), (ix, iy) = FREE_EDGES[name][:2]
    # a sensor inside the grid frees the cells around it either way; one outside frees nothing of the grid at equality
    # (the named tile is the nearest one) and one ulp above only the nearest cells, where they are not at lo already
    assert changed > 0 or not (0 <= ix < W and 0 <= iy < H)
    print("%s, %s max_range = %r: %d cells changed" % (name, which, scene["kw"]["max_range"], changed))


@pytest.mark.parametrize("name", ["edge of the tile, rotation 0", "edge of the tile, quarter turn",
                                  "first cell beyond, rotation 0", "first cell beyond, quarter turn", "45 degrees"])
def test_tile_at_the_boundary_of_can_hit(ops, name):
    scene, _ = hit_edge_scenes()[name]
    assert check_prior_scene(ops, scene, name) > 0


@pytest.mark.parametrize("i", range(G_SCENES))
def test_general_position(ops, i):
    scene, mag, small = general_scene(i)
    changed = check_prior_scene(ops, scene, i)
    print("scene %d: %d x %d, origin near %g, max_range %r: %d cells changed, every field the restatement's bits"
          % (i, scene["H"], scene["W"], MAGNITUDES[mag], scene["kw"]["max_range"], changed))


@pytest.mark.parametrize("name", ["N 1", "N 2", "N 3"])
def test_smallest_tables(ops, name):
    assert check_prior_scene(ops, small_table_scenes()[name], name) > 0


@pytest.fixture(scope="module")
def spoiled_scenes():
    return spoiled_pose_scenes()


@pytest.mark.parametrize("value", [v for v, _ in NON_FINITE])
@pytest.mark.parametrize("field", ["rot", "trans", "origin"])
def test_non_finite_pose_terms_leave_the_grid_alone(ops, spoiled_scenes, field, value):
    scene = spoiled_scenes[(field, value)]
    assert check_prior_scene(ops, scene, (field, value)) > 1000                # the healthy sensor's cells


# ------------------------------------------------------------------ B. the match
def check_family(ops, cases):
    for name, case in cases.items():
        check_case(ops, case, name)


def test_every_reach_from_0_to_16(ops):
    cases = reach_cases()
    assert len(cases) == 36
    check_family(ops, cases)


def test_long_scans_with_a_wide_search(ops):
    check_family(ops, long_scan_cases())


@pytest.mark.parametrize("k", range(len(PACK_SHAPES)), ids=["%d x %d" % s for s in PACK_SHAPES])
def test_packed_cells_on_the_borders_of_the_largest_grids(ops, k):
    H, W = PACK_SHAPES[k]
    got = check_case(ops, packing_case(H, W, 90 + k), "%d x %d" % (H, W))
    assert got["scores"].any()


def test_score_extremes_and_int64_gates(ops):
    cases = extreme_cases()
    assert len(cases) == 10
    check_family(ops, cases)


def test_equal_and_tied_candidates_at_the_largest_search(ops):
    cases = equal_cases()
    check_family(ops, cases)
    got = check_case(ops, cases["empty grid, room"], "empty grid, room")
    assert got["best"].tolist() == [[0, 0, 0]] and got["moved"].tolist() == [0] and got["scores"].shape == (1, 33, 33, 33)


def test_far_coordinates_one_beam_and_non_finite_terms(ops):
    cases = far_and_small_cases()
    assert len(cases) == 4 + 1 + 12
    check_family(ops, cases)
