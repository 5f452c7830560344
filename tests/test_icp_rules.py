"""The point-to-line ICP core (csrc/pof_icp.h) and the keyframe policies on top of it (keyframe_match.hip) where ties,
gates and pivots decide: the scene builders of tests/test_icp_rules_gpu.py and, without a GPU, the conditions those
scenes have to meet.  The referees are the restatements of tests/test_scan_match.py, tests/test_keyframe.py and
tests/test_keyframe_map.py, unchanged; what is new is the inputs and one small second referee.

Scenes whose arithmetic is exact.  The matchers read the angle table's (cos, sin) pairs as plain numbers, so a scene
writes its own table: beam i points along any dyadic pair d_i (not of unit length).  ``V(x, y)`` is a beam that carries
only a reference vertex at (x, y) (d = (x, y), reference range 1, current range not valid), ``P(x, y)`` only a current
point that the start value u puts at (x, y) (d = 2 ((x, y) - u), current range 0.5), ``VP`` both (u = 0), ``X`` neither;
ranges that are not valid cycle through NaN, +inf, 25 and 20 (== max_range).  All walls are axis-aligned, theta is 0 and
every matched point lies on its line, so every residual, the right-hand side and the step are exactly 0, the twelve sums
are exact in any order with or without FMA, and the pose keeps the bits of the start value.  tab[0] and tab[1] place
the window centres: dphi = 1024, so the beam-centred window of N9 / N10 is centred on ONE beam for every point of the
scene (tab[0] = -1024 (place + c_rel)), and the shift of N8 is 0.

The three conditions every (scene, entry point, placement) is held to:
  1. literal referee (``literal_core`` and ``literal_policy``, written from the header comments, one flag per rule): at
     the header's flags it gives the restatement's results, floats as equal values (NaN where NaN);
  2. exactness: every decision taken at a margin below MARGIN_MIN has both of its sides equal to their evaluation in
     ``fractions.Fraction`` from the float inputs (the squares of the settings -- gate2, gap2, key_dist2, rev_dist2 --
     count as inputs: one IEEE product on the host); every other decision keeps MARGIN_MIN, and the literal referee's
     smallest margins per kind are the restatement's;
  3. decisiveness: with the scene's one rule flipped the literal referee changes an exact output or state field, or a
     float by more than 1000 x the tolerance of the device comparison (1e-13).

rule -> scenes -> what the flipped rule changes
  nearest_upper (ties to the upper j / window scanned downwards)  tie_mid: corr; tie_lo, tie_hi (W = 2, the tied
                 vertices are the first and the last of the window): count
  gate_strict    gate_eq (d2 == gate2 == 1/64): count, corr; gate_zero: count 5 -> 0, ok      [gate_ulp: the other side]
  gap_strict     gap_eq (|e|^2 == gap2 == 1/64): count 5 -> 0, ok                             [gap_ulp: the other side]
  zero_edge      dup (a duplicate vertex on the j + 1 side): ok (a zero length poisons the sums); gap_zero (max_gap = 0
                 matches nothing): count 0 -> 1
  partner_plus   corner (equal legs, the point on the corner): obs
  partner_wrap   end_lo, end_hi (the only partner would be beam -1 / beam N): count, corr
  min_matches    three (a right-angle triple, also the smallest N that succeeds, N = 3): ok    [two, n1, n2: fail]
  pivot_ge       pivot0, pivot1, pivot2 (symmetric walls, diagonal A, min_pivot == p_k / dmax): ok, motion
                                               [pivot0_ulp, pivot1_ulp, pivot2_ulp: the other side, one ulp lower]
  stop_le        stop32 (eps = 0, zero step, iters = 32): iters_used 32 -> 1          [stop1: iters = 1; corner: 1e-7]
  window_off     win1 (N8) and win1_beam (N9, N10): vertices at mid +- 1 found, at mid +- 2 not: count 2 -> 4
  no_dphi_guard  dphi0 (tab[1] == tab[0]): count, ok
  keep_bad_init  bad_nan, bad_inf: count, ok
  left_ge        dist_eq (|u|^2 == key_dist2 == 1/16): key_replaced; hold_zero (key_dist = key_rot = 0, key_rel = 0)
                                                                                          [dist_ulp: the other side]
  stale_le       share_eq (matched == min_share votes): key_replaced          [share_more: one more point that votes]
  miss_ge        miss_keep (misses + 1 == max_misses): key_replaced, key_misses      [miss_over, miss_zero: re-anchor]
  revisit_lt     rev_eq (a stored keyframe at exactly rev_dist2), rev_zero (revisit = 0, a keyframe at the pose):
                 key_switched, key_slot                                                    [rev_ulp: the other side]
  winner_upper   rev_two (two keyframes at equal d2): key_slot
  lru_upper      lru (a full ring, equal stamps, the active slot 0): key_slot
  active_wrap    act_hi, act_lo (key_active = 9 and -2 with four slots): key_slot, ok
Scenes without a rule of their own (the other side of a rule scene, named in brackets above, or a limit that no flag
states): clamp_hi / clamp_lo (the shift of N8 clamps to +-N: empty windows, count 0; the restatement's own assertion
checks that nothing outside [0, N) is read), win64 (window = 64 on five beams) and alias (N8 from a start value
u = (0.25, 0), which the GPU test passes as the motion buffer of the same call).  ``keys = 1`` holds N9's bits on
every N9 scene (test_one_slot_is_the_keyframe_matcher_on_every_scene).

Placement.  Every scene runs at its own size (1 to 21 beams, the wave form), at the end of 512 beams, and in 513 and
4096 beams (the 512-thread form, slot layout t + 512 c) at beams 0.., across 511 / 512 / 513 and on the last beams;
every other beam is not valid.  The centre and shift margins stay near 0.5.

Left out on purpose.  Huber at |r| == huber_delta: both branches give w = 1, nothing can tell them apart.  |theta| at
key_rot or rev_rot with theta != 0: theta passes through sincos, so the scene cannot be made exact.  Anything that
would need a number read from the device: every boundary value comes from the scene's own exact arithmetic.

Measured without a GPU (``pytest tests/test_icp_rules.py --durations=0``, run alone): this file 9.3 s for 838 cases --
7.1 s the literal referee with its Fractions next to the restatement (2.2 to 2.7 s per entry point, 120 000
decisions, 6 700 of them at equality), 1.6 s the flipped runs, 0.3 s the sequential sums, the rest imports;
tests/test_grid_edges.py 6.9 s on the same machine."""
import math
from fractions import Fraction as Fr

import numpy as np
import pytest

from test_ego_motion import seq_sum
from test_keyframe import SETTINGS, keyframe_oracle, new_state
from test_keyframe_map import MAP, keyframe_map_oracle, new_map_state
from test_scan_match import DEFAULTS, MARGIN_MIN, match_oracle

E = 0.125
TOL = 1e-13                                                    # the floor of the project's tolerance rule: exact sums
DPHI = 1024.0
NOT_VALID = (np.nan, np.inf, 25.0, 20.0)
ENTRIES = ("scan_match", "keyframe", "keyframe_map")
HEADER = dict(nearest_upper=False, gate_strict=False, gap_strict=False, zero_edge=False, partner_plus=False,
              min_matches=3, pivot_ge=False, stop_le=False,
              # the limits around the core that the comments of scan_match.hip / keyframe_match.hip state
              window_off=0, partner_wrap=False, no_dphi_guard=False, keep_bad_init=False,
              # the policies of N9 and N10
              left_ge=False, stale_le=False, miss_ge=False, revisit_lt=False, winner_upper=False, lru_upper=False,
              active_wrap=False)
FLIPPED = dict({k: True for k, v in HEADER.items() if v is False}, min_matches=4, window_off=1)


# ================================================================ scenes
def V(x, y):
    return ((x, y), 1.0, None)


def P(x, y):
    return ((x, y), None, 0.5)


def VP(x, y):
    return ((x, y), 1.0, 1.0)


X = ((1.0, 0.0), None, None)
# the corner with equal legs: two walls of two edges each, the corner vertex in the middle
L5 = [VP(1, 1 - 2 * E), VP(1, 1 - E), VP(1, 1), VP(1 - E, 1), VP(1 - 2 * E, 1)]
L5V = [V(1, 1 - 2 * E), V(1, 1 - E), V(1, 1), V(1 - E, 1), V(1 - 2 * E, 1)]
L5P = [P(1, 1 - 2 * E), P(1, 1 - E), P(1, 1), P(1 - E, 1), P(1 - 2 * E, 1)]
ULP = lambda v: float(np.nextafter(v, 0.0))
SCENES = {}


def scene(name, rule, beams, entries=ENTRIES, other_side_of=None, why=None, **kw):
    assert name not in SCENES and (rule is None or rule in HEADER) and (rule or other_side_of or why)
    SCENES[name] = dict(name=name, rule=rule, beams=beams, entries=entries, other_side_of=other_side_of, why=why, **kw)


# ---------------------------------------------------------------- correspondence
scene("tie_mid", "nearest_upper", L5 + [X, V(2, 0), V(2, E), X, P(2, E / 2)])
# W = 2 around beam 3: the tied vertices are beam 1 (the window's first) and beam 5 (its last); only one has a partner
scene("tie_lo", "nearest_upper", [V(2, -E), V(2, 0), X, P(2, E), X, V(2, 2 * E), X], window=2, c_rel=3)
scene("tie_hi", "nearest_upper", [X, V(2, 0), X, P(2, E), X, V(2, 2 * E), V(2, 3 * E)], window=2, c_rel=3)
_gate = L5 + [X, V(2, -E), V(2, 0), X, P(2, E)]
scene("gate_eq", "gate_strict", _gate, gate=E)
scene("gate_ulp", None, _gate, other_side_of="gate_eq", gate=ULP(E))
scene("gate_zero", "gate_strict", _gate, gate=0.0)
scene("gap_eq", "gap_strict", L5, max_gap=E)
scene("gap_ulp", None, L5, other_side_of="gap_eq", max_gap=ULP(E))
_dup = L5 + [X, V(2, -E), V(2, 0), V(2, 0), X, P(2, 0)]
scene("dup", "zero_edge", _dup)
scene("gap_zero", "zero_edge", _dup, max_gap=0.0)
scene("corner", "partner_plus", L5)
# the only partner would be beam -1 (beam N): `ends` scenes put `beams` on the first and `tail` on the last beams
scene("end_lo", "partner_wrap", [V(2, 0), X] + L5 + [X, P(2, 0)], tail=[V(2, E)], centre="head")
scene("end_hi", "partner_wrap", [V(2, E)], tail=[P(2, 0), X] + L5 + [X, V(2, 0)], centre="tail")
# ---------------------------------------------------------------- iteration
scene("three", "min_matches", [VP(1, 1 - E), VP(1, 1), VP(1 - E, 1)])
scene("two", None, [X, VP(1, 1), VP(1 - E, 1)], other_side_of="three")
scene("n1", None, [VP(1, 1)], other_side_of="three", own_only=True)
scene("n2", None, [VP(1, 1), VP(1 - E, 1)], other_side_of="three", own_only=True)
scene("dphi0", "no_dphi_guard", L5 + [X] * 16, dphi=0.0, c_rel=0,
      forms=(("own", "own"), (512, "start"), (513, "start"), (4096, "start")))
_few = (("own", "own"), (512, "end"), (513, "wrap"), (4096, "end"))
scene("stop32", "stop_le", L5, eps_theta=0.0, eps_u=0.0, iters=32, forms=_few)
scene("stop1", None, L5, other_side_of="stop32", eps_theta=0.0, eps_u=0.0, iters=1)


def _walls(east_west, north_south):
    """Walls symmetric about both axes: x = +-1 with vertices at the y of `east_west`, y = +-1 at the x of
    `north_south` (one wall when a list is given as (values, "one")).  A is diagonal: A00 = sum y^2 + sum x^2, A11 and
    A22 the numbers of points."""
    out = []
    for sign in (1, -1):
        out += [VP(sign, y) for y in east_west] + [X]
    ns, sides = north_south if isinstance(north_south, tuple) else (north_south, "both")
    for sign in ((1, -1) if sides == "both" else (1,)):
        out += [VP(x, sign) for x in ns] + [X]
    return out[:-1]


_Q = (-0.75, -0.25, 0.25, 0.75)
# pivot -> (beams, min_pivot == p_k / dmax): A = diag(1.875, 8, 4) / diag(2.625, 2, 8) / diag(2.625, 8, 2)
PIVOTS = {0: (_walls((-0.5, -0.25, 0.25, 0.5), ((-0.5, -0.25, 0.25, 0.5), "one")), 15.0 / 64.0),
          1: ([((b[0][1], b[0][0]), b[1], b[2]) for b in _walls(_Q, ((-0.25, 0.25), "one"))], 0.25),
          2: (_walls(_Q, ((-0.25, 0.25), "one")), 0.25)}
for _k, (_beams, _mp) in PIVOTS.items():
    scene("pivot%d" % _k, "pivot_ge", _beams, max_gap=1.0, min_pivot=_mp)
    scene("pivot%d_ulp" % _k, None, _beams, other_side_of="pivot%d" % _k, max_gap=1.0, min_pivot=ULP(_mp))
# ---------------------------------------------------------------- windows and limits
scene("win1", "window_off", [P(2, 0), V(2, 0), V(2, E), X, P(3, 0), X, V(3, 0), V(3, E), X, V(4, E), V(4, 0), P(4, 0), X,
                             V(5, E), V(5, 0), X, P(5, 0)], entries=("scan_match",), window=1)
# beams 1, 2 | 4, 5 are mid - 2, mid - 1 | mid + 1, mid + 2 of the one centre; the gate keeps a point from its neighbour
scene("win1_beam", "window_off", [V(2, 2 * E), V(2, E), V(2, 0), X, V(3, 0), V(3, E), V(3, 2 * E), X, P(2, E), P(2, 0),
                                  P(3, 0), P(3, E)], entries=("keyframe", "keyframe_map"), window=1, c_rel=3, gate=E / 2)
scene("win64", None, L5, why="window = 64 on five beams: the clamp of the window to [0, N), which the restatement's "
      "own assertion checks", window=64)
_clamp = "the shift clamps to +-N: empty windows for the beams 16 or more from that end; " \
         "no flag states it, the restatement's assertion checks the reads"
scene("clamp_hi", None, [X] * 16 + L5, entries=("scan_match",), why=_clamp, init=(2.0 ** 40, 0.0, 0.0))
scene("clamp_lo", None, L5 + [X] * 16, entries=("scan_match",), why=_clamp, init=(-2.0 ** 40, 0.0, 0.0))
scene("alias", None, L5V + [X] + L5P, entries=("scan_match",), init=(0.0, 0.25, 0.0),
      why="the start value that the GPU test reads from the motion buffer of the same call")
scene("bad_nan", "keep_bad_init", L5, init=(0.0, np.nan, 0.0))
scene("bad_inf", "keep_bad_init", L5, init=(np.inf, 0.0, 0.0))
# ---------------------------------------------------------------- the keyframe policy (N9, and N10 with its ring)
KEYED = ("keyframe", "keyframe_map")
_moved = L5V + [X] + L5P                                        # the keyframe's corner seen from u = (0.25, 0)
scene("dist_eq", "left_ge", _moved, entries=KEYED, init=(0.0, 0.25, 0.0), key_dist=0.25)
scene("dist_ulp", None, _moved, entries=KEYED, other_side_of="dist_eq", init=(0.0, 0.25, 0.0), key_dist=ULP(0.25))
scene("hold_zero", "left_ge", L5, entries=KEYED, key_dist=0.0, key_rot=0.0)
_far = [P(9 + k, 9) for k in range(5)]                          # they vote and are beyond the gate
scene("share_eq", "stale_le", L5 + [X] + _far, entries=KEYED)
scene("share_more", None, L5 + [X] + _far + [P(15, 9)], entries=KEYED, other_side_of="share_eq")
_fails = [X, VP(1, 1), VP(1 - E, 1)]                            # two matched points: the match fails
scene("miss_keep", "miss_ge", _fails, entries=KEYED, key_misses=1)
scene("miss_over", None, _fails, entries=KEYED, other_side_of="miss_keep", key_misses=2)
scene("miss_zero", None, _fails, entries=KEYED, other_side_of="miss_keep", key_misses=0, max_misses=0)
# ---------------------------------------------------------------- the ring (N10): four slots, the pose ends at
# key_pose[active] + (0.25, 0); key_dist = 1/8, so the sensor has left and rev_dist2 = (1/16)^2
RING = ("keyframe_map",)
_ring = dict(entries=RING, init=(0.0, 0.25, 0.0), key_dist=E, key_pose=(0.5, -0.25, 0.0))
_at = lambda dx, dy=0.0: (0.75 + dx, -0.25 + dy, 0.0)           # a stored keyframe relative to where the pose ends
scene("rev_eq", "revisit_lt", _moved, stored={2: _at(E / 2)}, **_ring)
scene("rev_ulp", None, _moved, other_side_of="rev_eq", stored={2: _at(E / 2)}, revisit=ULP(0.5), **_ring)
scene("rev_zero", "revisit_lt", _moved, stored={2: _at(0.0)}, revisit=0.0, **_ring)
scene("rev_two", "winner_upper", _moved, stored={0: _at(E / 4), 3: _at(0.0, -E / 4)}, **_ring)
scene("lru", "lru_upper", _moved, stored={1: _at(5.0), 2: _at(-5.0), 3: _at(0.0, 5.0)}, active=0, **_ring)
scene("act_hi", "active_wrap", L5, entries=RING, active=9, active_slot=3)
scene("act_lo", "active_wrap", L5, entries=RING, active=-2, active_slot=0)

FORMS = (("own", "own"), (512, "end"), (513, "start"), (513, "wrap"), (513, "end"), (4096, "start"), (4096, "wrap"),
         (4096, "end"))
KEYS = 4


def forms_of(sc):
    if sc.get("own_only"):
        return (("own", "own"),)
    if "tail" in sc:
        return (("own", "ends"), (512, "ends"), (513, "ends"), (4096, "ends"))
    return sc.get("forms", FORMS)


def _settings(sc, entry):
    base = {"scan_match": DEFAULTS, "keyframe": SETTINGS, "keyframe_map": MAP}[entry]
    return dict(base, **{k: sc[k] for k in base if k in sc})


_CASES = {}


def case(name, entry, N, where):
    """The inputs of scene `name` for `entry` in a scan of N beams ("own": the scene's own length) at `where` ->
    dict: tab [3N], r0 / r1 float32 [N] (reference and current ranges), init [3] or None, settings, state (N9: the
    dict of ``new_state``; N10: of ``new_map_state``, primed), place, beams (the scene's own beam indices)."""
    key = (name, entry, N, where)
    if key in _CASES:
        return _CASES[key]
    sc = SCENES[name]
    head, tail = sc["beams"], sc.get("tail", [])
    n = len(head) + len(tail) + (4 if tail else 0)
    N = n if N == "own" else N
    place = {"own": 0, "start": 0, "ends": 0, "end": N - n,
             "wrap": min(512 - min(sc.get("c_rel", n // 2), n - 2), N - n)}[where]
    where_of = {place + i: b for i, b in enumerate(head)}
    where_of.update({N - len(tail) + i: b for i, b in enumerate(tail)})
    init = sc.get("init")
    u = np.array(init[1:], np.float64) if init is not None and np.isfinite(init).all() else np.zeros(2)
    beam = np.arange(N)
    dirs = np.tile(np.array(X[0]), (N, 1))
    r0, r1 = np.array(NOT_VALID, np.float32)[beam % 4], np.array(NOT_VALID, np.float32)[(beam // 2 + 1) % 4]
    for i, ((dx, dy), a, b) in where_of.items():
        if a is None and b is not None:                        # P: the start value puts the point at (dx, dy)
            dx, dy = 2.0 * (dx - u[0]), 2.0 * (dy - u[1])
        dirs[i] = dx, dy
        r0[i] = r0[i] if a is None else a
        r1[i] = r1[i] if b is None else b
    dphi = sc.get("dphi", DPHI)
    c_rel = sc.get("c_rel", 8)
    centre = (N - 1 - 8 if sc.get("centre") == "tail" else place + c_rel)
    phi = -dphi * centre + dphi * np.arange(N)
    tab = np.concatenate([phi, dirs.reshape(-1)])
    out = dict(name=name, entry=entry, N=N, place=place, tab=tab, r0=r0, r1=r1, settings=_settings(sc, entry),
               init=None if init is None else np.array(init, np.float64), beams=sorted(where_of))
    key_pose = np.array(sc.get("key_pose", (0.5, -0.25, 0.0)))
    key_rel = np.zeros(3) if init is None else np.array(init, np.float64)
    primed = dict(key_rel=key_rel, key_age=np.int32(3), key_misses=np.int32(sc.get("key_misses", 0)),
                  pose=key_pose + np.array([E, -E, 0.0]))
    if entry == "keyframe":
        out["state"] = dict(new_state(N), key_ranges=r0, key_pose=key_pose, key_valid=np.uint8(1), **primed)
    elif entry == "keyframe_map":
        st = new_map_state(N, KEYS)
        a = sc.get("active_slot", min(max(sc.get("active", 1), 0), KEYS - 1))
        st["key_ranges"][:] = (np.arange(KEYS, dtype=np.float32) + 0.5)[:, None]
        st["key_ranges"][a], st["key_pose"][a], st["key_valid"][a] = r0, key_pose, 1
        for k, pose in sc.get("stored", {}).items():
            st["key_pose"][k], st["key_valid"][k] = pose, 1
        st["key_stamp"][:] = 7
        st.update(primed, key_active=np.int32(sc.get("active", 1)), step=np.int32(11))
        out["state"] = st
    _CASES[key] = out
    return out


def all_cases(entry=None, form=None):
    """-> [(name, entry, N, where)] of every committed (scene, entry point, placement)."""
    return [(name, e, N, where) for name, sc in SCENES.items() for e in sc["entries"] if entry in (None, e)
            for N, where in forms_of(sc) if form in (None, (N, where))]


# ================================================================ the project's restatement on a case
OUT_EXACT = ("count", "ok", "iters_used", "corr", "key_replaced", "key_switched", "key_slot")
OUT_SAME = ("motion", "rms", "flow_residual", "trans", "flow_trans", "rot")      # exact by construction
OUT_TOL = ("obs",)                                                             # through the Cholesky factor
STATE_SAME = ("key_ranges", "key_pose", "key_rel", "key_valid", "key_age", "key_misses", "pose", "key_stamp",
              "key_active", "step")
_WANT = {}


def restatement(c, **kw):
    """-> (state after or None, outputs) of the project's float64 restatement on case c."""
    if c["entry"] == "scan_match":
        return None, match_oracle(c["r0"], c["r1"], c["tab"], init=c["init"], **dict(c["settings"], **kw))
    oracle = keyframe_oracle if c["entry"] == "keyframe" else keyframe_map_oracle
    return oracle(c["r1"], c["tab"], c["state"], **dict(c["settings"], **kw))


def want(key):
    """The restatement's (state, outputs) of ``case(*key)``, computed once and left unchanged."""
    if key not in _WANT:
        _WANT[key] = restatement(case(*key))
    return _WANT[key]


def differences(got, ref, tol=0.0):
    """The fields in which (state, outputs) `got` departs from `ref`: discrete fields and the floats that are exact by
    construction as values (NaN where NaN), obs within `tol`.  -> {field: largest difference or True}."""
    out = {}
    for g, r in ((got[1], ref[1]), (got[0] or {}, ref[0] or {})):
        for k in r:
            if k == "margins":
                continue
            x, y = np.asarray(g[k]), np.asarray(r[k])
            if k in OUT_TOL and np.isfinite(x).all() and np.isfinite(y).all():
                if abs(float(x) - float(y)) > tol:
                    out[k] = abs(float(x) - float(y))
            elif x.shape != y.shape or not np.array_equal(x, y, equal_nan=True):
                out[k] = True if k in OUT_EXACT + STATE_SAME or x.shape != y.shape else \
                    float(np.nanmax(np.abs(np.where(np.isfinite(x) & np.isfinite(y), x - y, np.inf))))
    return out


# ================================================================ the literal referee
def _fr(v):
    return Fr(float(v)) if np.isfinite(v) else None


def _fsqrt(f):
    """The exact root of a Fraction that is a square, else None."""
    if f is None or f < 0:
        return None
    a, b = math.isqrt(f.numerator), math.isqrt(f.denominator)
    return Fr(a, b) if a * a == f.numerator and b * b == f.denominator else None


def _ex(fn, *args):
    """fn over Fractions; None when an argument is None or the value is not rational."""
    try:
        return None if any(a is None for a in args) else fn(*args)
    except ZeroDivisionError:
        return None


class Log(list):
    """The decisions of one literal run: (kind, margin, left, right, left exact, right exact)."""

    def take(self, kind, margin, lhs, rhs, lhs_exact, rhs_exact):
        if np.isfinite(margin):
            self.append((kind, float(margin), lhs, rhs, lhs_exact, rhs_exact))

    def smallest(self):
        out = {}
        for kind, margin, *_ in self:
            out[kind] = min(out.get(kind, np.inf), margin)
        return out

    def assert_exact_or_clear(self, what):
        for kind, margin, lhs, rhs, le, re in self:
            if margin >= MARGIN_MIN:
                continue
            assert le is not None and re is not None, (what, kind, margin, lhs, rhs)
            assert Fr(float(lhs)) == le and Fr(float(rhs)) == re, (what, kind, lhs, rhs, le, re)


def _window_centre(entry, tab, N, F):
    """-> mid(i, qx, qy, th, log): the window centre of point i, by the comments of scan_match.hip (the beam shift)
    and keyframe_match.hip (the beam the transformed point falls on)."""
    phi0 = tab[0]
    dphi = tab[1] - tab[0] if N > 1 else 0.0

    def clamp(t, lo, hi, q, kind, log):
        if not t >= lo:                                         # a NaN gives the lower limit
            t = lo
        if not t <= hi:
            t = hi
        if np.isfinite(q):
            log.take(kind, abs(abs(q - np.floor(q)) - 0.5), q, 0.5, None, None)
        return int(t)

    def shift(i, qx, qy, th, log):
        if dphi == 0.0 and not F["no_dphi_guard"]:
            return i
        with np.errstate(all="ignore"):
            q = np.float64(th) / np.float64(dphi)
            return i + clamp(np.rint(q), -N, N, q, "shift", log)

    def beam(i, qx, qy, th, log):
        if dphi == 0.0 and not F["no_dphi_guard"]:
            return 0
        with np.errstate(all="ignore"):
            q = (np.arctan2(qy, qx) - phi0) / np.float64(dphi)
            return clamp(np.rint(q), -N, 2 * N, q, "centre", log)

    return shift if entry == "scan_match" else beam


def literal_correspond(ax, ay, N, W, gate2, gap2, mid, q, qF, F, log):
    """One point at q: -> (j, d, n, the exact n and d or None) or None when unmatched."""
    qx, qy = q
    best, bd, seen = -1, np.inf, []
    for j in range(max(mid - W, 0), min(mid + W, N - 1) + 1):   # upwards
        if np.isnan(ax[j]):
            continue
        dx, dy = qx - ax[j], qy - ay[j]
        d2 = dx * dx + dy * dy
        seen.append((j, d2))
        if d2 < bd or (F["nearest_upper"] and d2 == bd):
            best, bd = j, d2
    if best < 0:
        return None
    d2F = lambda j: _ex(lambda x, y, a, b: (x - a) ** 2 + (y - b) ** 2, qF[0], qF[1], _fr(ax[j]), _fr(ay[j]))
    bdF = d2F(best)
    for j, d2 in seen:
        if j != best and bd <= gate2:
            log.take("nearest", d2 - bd, d2, bd, d2F(j), bdF)
    log.take("gate", abs(bd - gate2), bd, gate2, bdF, Fr(gate2))
    if not (bd < gate2 if F["gate_strict"] else bd <= gate2):
        return None
    k, kd, e, l2, both = -1, 0.0, None, 0.0, []
    for side in ((1, -1) if F["partner_plus"] else (-1, 1)):    # the first side keeps a tie
        kk = best + side
        if F["partner_wrap"]:
            kk %= N
        if kk < 0 or kk >= N or np.isnan(ax[kk]):
            continue
        fx, fy = ax[kk] - ax[best], ay[kk] - ay[best]
        f2 = fx * fx + fy * fy
        f2F = _ex(lambda a, b, c, d: (a - c) ** 2 + (b - d) ** 2, _fr(ax[kk]), _fr(ay[kk]), _fr(ax[best]), _fr(ay[best]))
        log.take("edge", f2, f2, 0.0, f2F, Fr(0))
        if not (f2 > 0.0 or F["zero_edge"]):
            continue
        if f2 > 0.0:
            log.take("gap", abs(f2 - gap2), f2, gap2, f2F, Fr(gap2))
        if not (f2 < gap2 if F["gap_strict"] else f2 <= gap2):
            continue
        gx, gy = qx - ax[kk], qy - ay[kk]
        g2 = gx * gx + gy * gy
        both.append((g2, d2F(kk)))
        if k < 0 or g2 < kd:
            k, kd, e, l2 = kk, g2, (fx, fy), f2
    if len(both) == 2:
        log.take("partner", abs(both[0][0] - both[1][0]), both[0][0], both[1][0], both[0][1], both[1][1])
    if k < 0:
        return None
    with np.errstate(all="ignore"):
        length = np.sqrt(np.float64(l2))
        n = (-np.float64(e[1]) / length, np.float64(e[0]) / length)
    d = (qx - ax[best], qy - ay[best])
    lenF = _fsqrt(_ex(lambda a, b: a * a + b * b, _fr(e[0]), _fr(e[1])))
    nF = (_ex(lambda a, l: -a / l, _fr(e[1]), lenF), _ex(lambda a, l: a / l, _fr(e[0]), lenF))
    dF = (_ex(lambda a, b: a - b, qF[0], _fr(ax[best])), _ex(lambda a, b: a - b, qF[1], _fr(ay[best])))
    return best, d, n, nF, dF


def literal_core(c, init, F, log):
    """The comment of pof_icp.h, point by point: the iterations from `init` and the final correspondence pass.
    -> failed, (theta, u), count, rms, iters_used, obs, corr [N], flow_residual [N,2], whether the pose kept the
    bits of init."""
    N, tab, st = c["N"], c["tab"], c["settings"]
    cs, sn = tab[N::2], tab[N + 1::2]
    with np.errstate(all="ignore"):
        r0, r1 = c["r0"].astype(np.float64), c["r1"].astype(np.float64)
        v0 = np.isfinite(r0) & (r0 < st["max_range"])
        valid = np.isfinite(r1) & (r1 < st["max_range"])
        ax, ay = np.where(v0, r0 * cs, np.nan), np.where(v0, r0 * sn, np.nan)
        px, py = r1 * cs, r1 * sn
    for i in np.flatnonzero(v0 | valid):                       # the staged products are exact
        assert not v0[i] or (Fr(float(ax[i])), Fr(float(ay[i]))) == (Fr(float(r0[i])) * Fr(cs[i]), Fr(float(r0[i])) * Fr(sn[i]))
        assert not valid[i] or (Fr(float(px[i])), Fr(float(py[i]))) == (Fr(float(r1[i])) * Fr(cs[i]), Fr(float(r1[i])) * Fr(sn[i]))
    W = st["window"] + F["window_off"]
    gate2, gap2 = st["gate"] * st["gate"], st["max_gap"] * st["max_gap"]
    hd, min_pivot = st["huber_delta"], st["min_pivot"]
    centre = _window_centre(c["entry"], tab, N, F)
    th, ux, uy = (np.float64(v) for v in init)
    still = True                                                # the pose still has the bits of init

    def points(log):
        co, si = np.cos(th), np.sin(th)
        for i in np.flatnonzero(valid):
            with np.errstate(all="ignore"):
                q = ((co * px[i] - si * py[i]) + ux, (si * px[i] + co * py[i]) + uy)
            qF = (_ex(lambda a, b, p0, p1, u0: (a * p0 - b * p1) + u0, _fr(co), _fr(si), _fr(px[i]), _fr(py[i]), _fr(ux)),
                  _ex(lambda a, b, p0, p1, u0: (b * p0 + a * p1) + u0, _fr(co), _fr(si), _fr(px[i]), _fr(py[i]), _fr(uy)))
            mid = centre(int(i), q[0], q[1], th, log)
            with np.errstate(all="ignore"):
                hit = literal_correspond(ax, ay, N, W, gate2, gap2, mid, q, qF, F, log)
            if hit is not None:
                yield (int(i), q, qF) + hit

    failed, used, count, rms, obs = False, 0, 0, np.nan, 0.0
    with np.errstate(all="ignore"):
        for it in range(int(st["iters"])):
            S, SF = [np.float64(0.0)] * 12, [Fr(0)] * 9
            for i, q, qF, j, d, n, nF, dF in points(log):
                r = n[0] * d[0] + n[1] * d[1]
                rF = _ex(lambda a, b, e, f: a * e + b * f, nF[0], nF[1], dF[0], dF[1])
                ar = abs(r)
                if hd > 0.0:
                    log.take("huber", abs(ar - hd), ar, hd, _ex(abs, rF), Fr(hd))
                w = hd / ar if hd > 0.0 and ar > hd else 1.0
                J = (n[0] * (-q[1]) + n[1] * q[0], n[0], n[1])
                JF = (_ex(lambda a, b, x, y: a * (-y) + b * x, nF[0], nF[1], qF[0], qF[1]), nF[0], nF[1])
                terms = [w * (J[a] * J[b]) for a in range(3) for b in range(a, 3)] + [w * (J[a] * r) for a in range(3)]
                termsF = [_ex(lambda x, y: x * y, JF[a], JF[b]) if w == 1.0 else None for a in range(3) for b in range(a, 3)] + \
                         [_ex(lambda x, y: x * y, JF[a], rF) if w == 1.0 else None for a in range(3)]
                for t in range(9):
                    S[t] = S[t] + terms[t]
                    SF[t] = _ex(lambda x, y: x + y, SF[t], termsF[t])
                S[9], S[10], S[11] = S[9] + w, S[10] + w * (r * r), S[11] + 1.0
            used, count = it + 1, int(S[11])
            rms = np.sqrt(S[10] / S[9])
            if count < F["min_matches"]:
                failed, obs = True, 0.0
                break
            dmax = max(S[0], max(S[3], S[5]))
            floor_ = min_pivot * dmax
            floorF = _ex(lambda a, b, cc: Fr(min_pivot) * max(a, b, cc), SF[0], SF[3], SF[5])
            passes = lambda p: p >= floor_ if F["pivot_ge"] else p > floor_
            # the exact pivots are those of the LDL^T factorisation, which are rational
            p1F = _ex(lambda a00, a01, a11: a11 - a01 * a01 / a00, SF[0], SF[1], SF[3])
            p2F = _ex(lambda a00, a01, a02, a12, a22, p1: a22 - a02 * a02 / a00 - (a12 - a02 * a01 / a00) ** 2 / p1,
                      SF[0], SF[1], SF[2], SF[4], SF[5], p1F)
            pivots, l = [S[0]], {}
            log.take("pivot", abs(pivots[0] / dmax - min_pivot) if dmax > 0.0 else np.inf, pivots[0], floor_, SF[0], floorF)
            failed = not passes(pivots[0])
            if not failed:
                l[0, 0] = np.sqrt(pivots[0])
                l[1, 0], l[2, 0] = S[1] / l[0, 0], S[2] / l[0, 0]
                pivots.append(S[3] - l[1, 0] * l[1, 0])
                log.take("pivot", abs(pivots[1] / dmax - min_pivot), pivots[1], floor_, p1F, floorF)
                failed = not passes(pivots[1])
                if not failed:
                    l[1, 1] = np.sqrt(pivots[1])
                    l[2, 1] = (S[4] - l[2, 0] * l[1, 0]) / l[1, 1]
                    pivots.append((S[5] - l[2, 0] * l[2, 0]) - l[2, 1] * l[2, 1])
                    log.take("pivot", abs(pivots[2] / dmax - min_pivot), pivots[2], floor_, p2F, floorF)
                    failed = not passes(pivots[2])
                    if not failed:
                        l[2, 2] = np.sqrt(pivots[2])
            obs = min(pivots) / dmax if dmax > 0.0 else 0.0
            if failed:
                break
            y0 = -S[6] / l[0, 0]
            y1 = (-S[7] - l[1, 0] * y0) / l[1, 1]
            y2 = ((-S[8] - l[2, 0] * y0) - l[2, 1] * y1) / l[2, 2]
            x2 = y2 / l[2, 2]
            x1 = (y1 - l[2, 1] * x2) / l[1, 1]
            x0 = ((y0 - l[1, 0] * x1) - l[2, 0] * x2) / l[0, 0]
            c0, s0 = np.cos(x0), np.sin(x0)
            th, ux, uy = th + x0, (c0 * ux - s0 * uy) + x1, (s0 * ux + c0 * uy) + x2
            zero = Fr(0) if SF[6] == 0 and SF[7] == 0 and SF[8] == 0 else None      # a zero right-hand side: a zero step
            still = still and zero is not None and x0 == 0.0 and x1 == 0.0 and x2 == 0.0
            log.take("stop", abs(abs(x0) - st["eps_theta"]), abs(x0), st["eps_theta"], zero, Fr(st["eps_theta"]))
            log.take("stop", abs(max(abs(x1), abs(x2)) - st["eps_u"]), max(abs(x1), abs(x2)), st["eps_u"], zero, Fr(st["eps_u"]))
            small = (lambda a, b: a <= b) if F["stop_le"] else (lambda a, b: a < b)
            if small(abs(x0), st["eps_theta"]) and small(max(abs(x1), abs(x2)), st["eps_u"]):
                break
        corr, res = np.full(N, -1, np.int32), np.full((N, 2), np.nan)
        if not failed:
            co, si = np.cos(th), np.sin(th)
            for i, q, qF, j, d, n, nF, dF in points(log):
                corr[i] = j
                res[i] = co * d[0] + si * d[1], (-si) * d[0] + co * d[1]
    return failed, np.array([th, ux, uy]), count, rms, used, obs, corr, res, still


def _start(init, F):
    init = np.zeros(3) if init is None else np.asarray(init, np.float64)
    return init if np.isfinite(init).all() or F["keep_bad_init"] else np.zeros(3)


def literal(c, **flips):
    """Case c through the literal referee with the header's flags but `flips` -> (state after or None, outputs, log)."""
    F, log = dict(HEADER, **flips), Log()
    nan, N = np.nan, c["N"]
    if c["entry"] == "scan_match":
        failed, m, count, rms, used, obs, corr, res, _ = literal_core(c, _start(c["init"], F), F, log)
        return None, {"motion": np.full(3, nan) if failed else m, "ok": np.uint8(not failed), "count": np.int32(count),
                      "rms": nan if failed else float(rms), "iters_used": np.int32(used), "obs": float(obs), "corr": corr,
                      "flow_residual": res}, log
    return literal_policy(c, F, log) + (log,)


def literal_policy(c, F, log):
    """The N9 / N10 comments: the keyframe policy around ``literal_core``.  N9 is the ring of one slot."""
    st, N, ring = c["settings"], c["N"], c["entry"] == "keyframe_map"
    s = {k: np.copy(v) for k, v in c["state"].items()}
    if not ring:                                                # N9's state as a ring of one slot
        s.update(key_ranges=s["key_ranges"][None], key_pose=s["key_pose"][None], key_valid=s["key_valid"][None],
                 key_stamp=np.zeros(1, np.int32), key_active=np.int32(0), step=np.int32(0))
    K = len(s["key_valid"])
    a = int(s["key_active"])
    a = a % K if F["active_wrap"] else min(max(a, 0), K - 1)
    r1 = c["r1"]
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(r1) & (r1.astype(np.float64) < st["max_range"])
    gated = np.where(valid, r1, np.float32(np.nan)).astype(np.float32)
    votes = int(valid.sum())
    old = s["pose"].astype(np.float64).copy()
    pose, nan3 = old.copy(), np.full(3, np.nan)
    out = dict(motion=nan3, ok=np.uint8(0), count=np.int32(0), rms=np.nan, iters_used=np.int32(0), obs=0.0,
               corr=np.full(N, -1, np.int32), flow_residual=np.full((N, 2), np.nan))
    store, switched, slot, rel_new = False, False, a, None
    age, misses = int(s["key_age"]), int(s["key_misses"])
    if not s["key_valid"][a]:
        store, age, misses = True, 0, 0
    else:
        failed, rel, count, rms, used, obs, corr, res, still = literal_core(
            dict(c, r0=s["key_ranges"][a]), _start(s["key_rel"], F), F, log)
        out.update(count=np.int32(count), iters_used=np.int32(used), obs=float(obs), corr=corr, flow_residual=res)
        if failed:
            store = misses + 1 >= st["max_misses"] if F["miss_ge"] else misses + 1 > st["max_misses"]
            age, misses = (0, 0) if store else (age + 1, misses + 1)
        else:
            out.update(motion=rel, ok=np.uint8(1), rms=float(rms))
            key = s["key_pose"][a].astype(np.float64)
            ck, sk = np.cos(key[2]), np.sin(key[2])
            pose = np.array([key[0] + (ck * rel[1] - sk * rel[2]), key[1] + (sk * rel[1] + ck * rel[2]), key[2] + rel[0]])
            relF = [_fr(v) if still else None for v in rel]
            level = key[2] == 0.0 and still                    # then the pose is key + u exactly
            poseF = [_ex(lambda p, q: p + q, _fr(key[0]), relF[1]), _ex(lambda p, q: p + q, _fr(key[1]), relF[2])] \
                if level else [None, None]
            u2, d2 = rel[1] * rel[1] + rel[2] * rel[2], st["key_dist"] * st["key_dist"]
            u2F = _ex(lambda p, q: p * p + q * q, relF[1], relF[2])
            log.take("key_rot", abs(abs(rel[0]) - st["key_rot"]), abs(rel[0]), st["key_rot"], _ex(abs, relF[0]), Fr(st["key_rot"]))
            log.take("key_dist", abs(u2 - d2), u2, d2, u2F, Fr(d2))
            share = st["min_share"] * float(votes)
            log.take("min_share", abs(float(count) - share), float(count), share, Fr(count), Fr(st["min_share"]) * votes)
            more = (lambda p, q: p >= q) if F["left_ge"] else (lambda p, q: p > q)
            left = bool(more(abs(rel[0]), st["key_rot"]) or more(u2, d2))
            stale = bool(float(count) <= share if F["stale_le"] else float(count) < share)
            age, misses, rel_new = (0 if left or stale else age + 1), 0, rel.copy()
            store = left or stale
            if left and ring:
                rev_rot = st["revisit"] * st["key_rot"]
                rev_d2 = (st["revisit"] * st["key_dist"]) * (st["revisit"] * st["key_dist"])
                win, win_d2, winF, free, lru = -1, 0.0, None, -1, -1
                for k in range(K):                              # in ascending k
                    if not s["key_valid"][k]:
                        free = k if free < 0 else free
                        continue
                    if k == a:
                        continue
                    stamp = int(s["key_stamp"][k])
                    if lru < 0 or stamp < int(s["key_stamp"][lru]) or (F["lru_upper"] and stamp == int(s["key_stamp"][lru])):
                        lru = k
                    pk = s["key_pose"][k].astype(np.float64)
                    t = math.remainder(float(pose[2]) - float(pk[2]), 2.0 * math.pi)
                    dx, dy = pose[0] - pk[0], pose[1] - pk[1]
                    c1, s1 = np.cos(pk[2]), np.sin(pk[2])
                    vx, vy = c1 * dx + s1 * dy, (-s1) * dx + c1 * dy
                    c2 = vx * vx + vy * vy
                    flat = pk[2] == 0.0 and pose[2] == 0.0
                    c2F = _ex(lambda p, q, x, y: (p - x) ** 2 + (q - y) ** 2, poseF[0], poseF[1], _fr(pk[0]), _fr(pk[1])) \
                        if flat else None
                    log.take("revisit_rot", abs(abs(t) - rev_rot), abs(t), rev_rot, Fr(0) if flat else None, Fr(rev_rot))
                    log.take("revisit_dist", abs(c2 - rev_d2), c2, rev_d2, c2F, Fr(rev_d2))
                    inside = (lambda p, q: p < q) if F["revisit_lt"] else (lambda p, q: p <= q)
                    if inside(abs(t), rev_rot) and inside(c2, rev_d2):
                        if win >= 0:
                            log.take("winner", abs(c2 - win_d2), c2, win_d2, c2F, winF)
                        if win < 0 or c2 < win_d2 or (F["winner_upper"] and c2 == win_d2):
                            win, win_d2, winF, rel_new = k, c2, c2F, np.array([t, vx, vy])
                if win >= 0:
                    store, switched, slot = False, True, win
                else:
                    slot = free if free >= 0 else (lru if lru >= 0 else a)
    if store:
        s["key_ranges"][slot], s["key_pose"][slot], s["key_valid"][slot] = gated, pose, 1
        s["key_rel"] = np.zeros(3)
    elif rel_new is not None:
        s["key_rel"] = rel_new.copy()
    s["key_stamp"][slot] = s["step"]
    s.update(key_active=np.int32(slot), key_age=np.int32(age), key_misses=np.int32(misses),
             step=np.int32(int(s["step"]) + 1), pose=pose.copy())
    c1, s1 = np.cos(pose[2]), np.sin(pose[2])
    good = bool(out["ok"])
    out.update(key_replaced=np.uint8(store), rot=np.array([c1, -s1, s1, c1]).astype(np.float32), trans=pose[:2].copy(),
               flow_trans=(pose[:2] - old[:2]) if good else np.zeros(2))
    if ring:
        out.update(key_switched=np.uint8(switched), key_slot=np.int32(slot))
    else:
        s = dict({k: v for k, v in s.items() if k not in ("key_stamp", "key_active", "step")},
                 key_ranges=s["key_ranges"][0], key_pose=s["key_pose"][0], key_valid=np.uint8(1))
    return s, out


# ================================================================ tests (no GPU)
COMPARED = ("nearest", "gate", "gap", "partner", "pivot", "stop", "huber", "shift", "centre", "key_rot", "key_dist",
            "min_share", "revisit_rot", "revisit_dist", "winner")


def _ids(keys):
    return ["%s-%s-%s-%s" % k for k in keys]


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_literal_referee_is_the_restatement_and_every_close_decision_is_exact(entry):
    decisions, close = 0, 0
    for key in all_cases(entry):
        ref = want(key)
        state, out, log = literal(case(*key))
        assert differences((state, out), ref) == {}, (key, differences((state, out), ref))
        assert set(ref[1]) - {"margins"} == set(out) and (state is None or set(state) == set(ref[0])), key
        log.assert_exact_or_clear(key)
        mine, theirs = log.smallest(), ref[1]["margins"]
        for kind in COMPARED:
            assert mine.get(kind, np.inf) == theirs.get(kind, np.inf), (key, kind, mine.get(kind), theirs.get(kind))
        assert set(theirs) - {"decisions"} <= set(COMPARED), theirs.keys()
        for kind in ("shift", "centre"):
            assert mine.get(kind, np.inf) >= 0.25, (key, kind, mine[kind])
        decisions, close = decisions + len(log), close + sum(m < MARGIN_MIN for _, m, *_ in log)
    print("%s: %d cases, %d decisions, %d of them below MARGIN_MIN and exact" % (entry, len(all_cases(entry)), decisions, close))
    assert close > 0


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_scene_is_decided_by_its_rule(entry):
    for key in all_cases(entry):
        sc, ref = SCENES[key[0]], want(key)
        if sc["rule"] is None:
            assert sc["why"] or sc["other_side_of"] in SCENES
            if sc["other_side_of"] and SCENES[sc["other_side_of"]].get("own_only") == sc.get("own_only") \
                    and forms_of(SCENES[sc["other_side_of"]]) == forms_of(sc):
                # the other side shows: an exact output or state field differs from the rule scene's
                twin = want((sc["other_side_of"],) + key[1:])
                changed = differences(ref, twin)
                assert any(v is True for k, v in changed.items() if k not in ("key_ranges",)), (key, changed)
            continue
        state, out, _ = literal(case(*key), **{sc["rule"]: FLIPPED[sc["rule"]]})
        changed = differences((state, out), ref, tol=1000.0 * TOL)
        assert any(v is True or v > 1000.0 * TOL for v in changed.values()), (key, sc["rule"], changed)


def test_the_sums_are_exact_so_the_tolerance_rule_gives_its_floor():
    """The project's rule -- 100 x the disagreement of the pairwise and the sequential evaluation, at least 1e-13 -- on
    these scenes: the two agree in every bit, so TOL is the floor."""
    for form in (("own", "own"), ("own", "ends"), (513, "wrap")):
        for key in all_cases(form=form):
            assert differences(restatement(case(*key), sum=seq_sum), want(key)) == {}, key
    assert max(1e-13, 100.0 * 0.0) == TOL <= 1e-10


def test_the_scenes_do_what_their_names_say():
    """The restatement's results on the scenes at their own size: what the table of the docstring claims."""
    o = lambda name, entry="scan_match", **kw: want((name, entry) + forms_of(SCENES[name])[0])[1]
    s = lambda name, entry: want((name, entry) + forms_of(SCENES[name])[0])[0]
    assert o("tie_mid")["ok"] and o("tie_mid")["corr"][9] == 6 and o("tie_mid")["count"] == 6
    assert o("tie_lo")["count"] == 1 and o("tie_hi")["count"] == 0
    assert o("gate_eq")["count"] == 6 and o("gate_ulp")["count"] == 5 and o("gate_zero")["count"] == 5
    assert o("gate_eq")["corr"][9] == 7 and o("gate_zero")["ok"]
    assert o("gap_eq")["count"] == 5 and o("gap_eq")["ok"] and o("gap_ulp")["count"] == 0 and not o("gap_ulp")["ok"]
    assert o("dup")["ok"] and o("dup")["count"] == 6 and o("dup")["corr"][10] == 7
    assert o("gap_zero")["count"] == 0 and not o("gap_zero")["ok"]
    assert o("corner")["ok"] and o("corner")["count"] == 5 and o("corner")["iters_used"] == 1
    assert o("end_lo")["count"] == 5 and o("end_lo")["corr"][8] == -1 and o("end_hi")["count"] == 5
    assert o("three")["ok"] and o("three")["count"] == 3
    assert not o("two")["ok"] and o("two")["count"] == 2 and o("two")["obs"] == 0.0
    assert not o("n1")["ok"] and o("n1")["count"] == 0 and not o("n2")["ok"] and o("n2")["count"] == 2
    assert o("dphi0")["ok"] and o("dphi0", "keyframe")["ok"]
    assert o("stop32")["iters_used"] == 32 and o("stop1")["iters_used"] == 1 and o("stop32")["ok"]
    for k, (_, mp) in PIVOTS.items():
        fail, ok = o("pivot%d" % k), o("pivot%d_ulp" % k)
        assert not fail["ok"] and fail["obs"] == mp and fail["count"] == ok["count"] and ok["ok"] and ok["obs"] == mp, k
        assert np.array_equal(ok["motion"], np.zeros(3))
    assert o("win1")["count"] == 2 and o("win1_beam", "keyframe")["count"] == 2
    assert o("win64")["ok"] and o("win64")["count"] == 5
    assert o("alias")["ok"] and np.array_equal(o("alias")["motion"], [0.0, 0.25, 0.0]) and o("alias")["count"] == 5
    for name in ("clamp_hi", "clamp_lo"):
        assert o(name)["count"] == 0 and not o(name)["ok"] and o(name)["iters_used"] == 1
    for name in ("bad_nan", "bad_inf"):
        for entry in ENTRIES:
            assert o(name, entry)["ok"] and np.array_equal(o(name, entry)["motion"], np.zeros(3))
    for entry in KEYED:
        assert np.array_equal(o("dist_eq", entry)["motion"], [0.0, 0.25, 0.0]) and o("dist_eq", entry)["iters_used"] == 1
        assert not o("dist_eq", entry)["key_replaced"] or entry == "keyframe_map"
        assert o("hold_zero", entry)["ok"] and not o("hold_zero", entry)["key_replaced"]
        assert o("share_eq", entry)["count"] == 5 and not o("share_eq", entry)["key_replaced"]
        assert o("share_more", entry)["count"] == 5 and o("share_more", entry)["key_replaced"]
        assert not o("miss_keep", entry)["ok"] and not o("miss_keep", entry)["key_replaced"]
        assert s("miss_keep", entry)["key_misses"] == 2 and s("miss_keep", entry)["key_age"] == 4
        assert o("miss_over", entry)["key_replaced"] and s("miss_over", entry)["key_misses"] == 0
        assert o("miss_zero", entry)["key_replaced"] and not o("miss_zero", entry)["ok"]
    assert not o("dist_eq", "keyframe")["key_replaced"] and o("dist_ulp", "keyframe")["key_replaced"]
    assert not o("dist_eq", "keyframe_map")["key_replaced"] and o("dist_ulp", "keyframe_map")["key_replaced"]
    m = lambda name: o(name, "keyframe_map")
    assert m("rev_eq")["key_switched"] and m("rev_eq")["key_slot"] == 2 and not m("rev_eq")["key_replaced"]
    assert np.array_equal(s("rev_eq", "keyframe_map")["key_rel"], [0.0, -E / 2, 0.0])
    assert not m("rev_ulp")["key_switched"] and m("rev_ulp")["key_replaced"] and m("rev_ulp")["key_slot"] == 0
    assert m("rev_zero")["key_switched"] and m("rev_zero")["key_slot"] == 2
    assert m("rev_two")["key_switched"] and m("rev_two")["key_slot"] == 0
    assert m("lru")["key_replaced"] and m("lru")["key_slot"] == 1 and not m("lru")["key_switched"]
    assert m("act_hi")["ok"] and m("act_hi")["key_slot"] == 3 and m("act_lo")["ok"] and m("act_lo")["key_slot"] == 0


def test_one_slot_is_the_keyframe_matcher_on_every_scene():
    """keys = 1: the ring's restatement leaves N9's results on every N9 scene at its own size."""
    for key in all_cases("keyframe", ("own", "own")) + all_cases("keyframe", ("own", "ends")):
        c = case(*key)
        state, out = want(key)
        ring = dict(new_map_state(c["N"], 1), key_ranges=c["state"]["key_ranges"][None].copy(),
                    key_pose=c["state"]["key_pose"][None].copy(), key_valid=np.ones(1, np.uint8),
                    **{k: c["state"][k] for k in ("key_rel", "key_age", "key_misses", "pose")})
        rs, ro = keyframe_map_oracle(c["r1"], c["tab"], ring, **dict(c["settings"], revisit=0.5))
        for k in out:
            assert k == "margins" or np.array_equal(ro[k], out[k], equal_nan=True), (key, k)
        for k in state:
            assert np.array_equal(np.asarray(rs[k]).reshape(np.shape(state[k])), state[k], equal_nan=True), (key, k)
        assert not ro["key_switched"] and ro["key_slot"] == 0


def test_every_rule_has_a_scene_for_every_entry_point_it_applies_to_and_the_left_out_rules_are_named():
    rules = {e: {sc["rule"] for sc in SCENES.values() if e in sc["entries"]} for e in ENTRIES}
    core = {k for k in HEADER if k not in ("left_ge", "stale_le", "miss_ge", "revisit_lt", "winner_upper", "lru_upper",
                                           "active_wrap")}
    assert core <= rules["scan_match"] and core <= rules["keyframe"] and core <= rules["keyframe_map"]
    assert {"left_ge", "stale_le", "miss_ge"} <= rules["keyframe"] and set(HEADER) <= rules["keyframe_map"]
    for word in ("Left out on purpose", "|r| == huber_delta", "key_rot or rev_rot", "read from the device"):
        assert word in __doc__, word
    for name, sc in SCENES.items():
        assert name in __doc__, name
