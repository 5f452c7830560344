"""Person motion (pof_person_motion, N11), person tracks (pof_track_update, N7) and the base weights of pof_ego_motion
(N6) where row slots, gates and ties decide: the scene builders, and what can be said about the scenes without a GPU.
tests/test_person_rules_gpu.py runs them on the device against the same restatements.

Why these scenes.  person_motion.hip keeps detection row k in thread k % T, register slot k / T (T = 64 for N <= 512,
512 above) and lets only the first ceil(num_det / T) and ceil(prev_num / T) slots take part in its two walks;
track_update.hip keeps track slot s in lane s % 64, register slot s / 64.  The rule scenes of tests/test_person_motion.py
use rows 0..7 and the tie scenes of tests/test_tracks.py tie slots of different lanes, so every rule was only ever taken
by the first slot of the first lanes.  Here the same scenes are replayed from detection row ``at`` on, behind ``at``
decoy rows that each pair with themselves (so every lower slot does real work), at placements that put the deciding
rows into slot >= 1, across the 63 | 64 and 511 | 512 ownership boundaries and into the last slot of either form; the
tracker gets ties between the slots of one lane, the gate at equality and at 0, max_misses = 0, a slot that loses
three cached candidates in a row, and candidates behind the first staged chunk of 1024.

Every coordinate is dyadic and exact in float32, so a tie is a tie of equal bits and every other decision has a margin
of at least 2^-20 m^2; the tests below assert that, and that each scene reaches the slot, lane and wave it is for.

Placements.  A two-point row (tests/test_person_motion.AxisScan.row) costs two beams, so ``at`` two-point decoys and
the 16 beams of the rules scene need 2 at + 16 <= N: (128, 60), (512, 448), (512, 500) and (1024, 505) cannot hold
two-point rows.  They run the single-point scene (``point_scans``, min_points = 1: 12 beams, three per axis), and the
two-point scenes run at (192, 60), (512, 64), (512, 120), (2048, 505), (4096, 512) and (4096, 2030).  Not reachable:
the rows 4094 and 4095 of a 4096-beam scan, because the single-point scene needs two beams for its left-out ranges.

The referees are person_motion_oracle (tests/test_person_motion.py), track_step (tests/test_tracks.py) and base_weights
(tests/test_ego_motion.py); nothing here restates a kernel.  Measured: the restatement takes 0.02-0.5 s per placed
sequence (the longest: N = 4096 with 4094 rows)."""
import numpy as np
import pytest

from test_ego_motion import base_weights, rigid_field
from test_person_motion import AXES, DEFAULTS, AxisScan, motion_state, rule_scans, run_axis, same_bits, tie_scans
from test_tracks import SETTINGS, run_steps, scan_of

MAX_RANGE = 2.0 ** 20                                          # dyadic, exact in float32, beyond every decoy
FAR = 2.0 * MAX_RANGE                                          # a beam that is nobody's
KW2 = dict(DEFAULTS, min_points=2, max_range=MAX_RANGE)        # the settings of the two-point scenes
KW1 = dict(DEFAULTS, min_points=1, max_range=MAX_RANGE)        # ... of the single-point scenes
MARGIN = 2.0 ** -20
below = lambda x: float(np.nextafter(np.float64(x), 0.0))
below32 = lambda x: float(np.nextafter(np.float32(x), np.float32(0.0)))


def threads_of(N):
    """The launcher's choice (csrc/pof_sensor.h): one wave up to 512 beams, 512 threads above."""
    return 64 if N <= 512 else 512


def owner(k, N):
    """(thread, register slot, wave) of detection row k in a launch of N beams."""
    T = threads_of(N)
    return k % T, k // T, (k % T) >> 6


# ---------------------------------------------------------------- 1. person motion: rows placed anywhere
def decoy(f, t, points=2):
    """Decoy f in scan t: centroid 64 + 2 (f // 4) + 0.125 t metres along AXES[f % 4] -- 2 m from the next decoy of its
    axis, 0.125 m from itself one scan earlier.  Two points (the second, None, is a zero-range point on whichever axis
    has beams left) or one."""
    c = 64.0 + 2.0 * (f // 4) + 0.125 * t
    ax = AXES[f % 4]
    return [(f % 4, points * c)] + [None] * (points - 1), 0.9, (c * ax[0], c * ax[1])


def xy_row(x, y, cls=0.9):
    """AxisScan.row as a row spec: the points (2x, 0) and (0, 2y), centroid (x, y)."""
    return [(0 if x >= 0 else 2, 2 * abs(x)), (1 if y >= 0 else 3, 2 * abs(y))], cls, (x, y)


def pt(axis, r, cls=0.9):
    """A single-point row at range r along AXES[axis]."""
    return [(axis, r)], cls, (r * AXES[axis][0], r * AXES[axis][1])


def place(N, entries, t=0, points=2):
    """One scan of N beams whose detection row k is entries[k]: an int f (decoy f of scan t, ``points`` points) or a
    row spec (points, cls, xy).  The stated points take the lowest free beams of their axes in row order, the decoys'
    zero-range points whatever is left; running out of beams raises.  -> AxisScan."""
    s = AxisScan(N)
    s.ranges[:] = FAR
    filler = []
    for e in entries:
        pts, cls, xy = decoy(int(e), t, points) if isinstance(e, (int, np.integer)) else e
        k = s.row_points([p for p in pts if p is not None], cls, xy)
        filler += [k] * sum(p is None for p in pts)
    for k in filler:
        axis = max(range(4), key=lambda a: len(s.free[a]))
        i = s.free[axis].pop(0)
        s.ranges[i], s.inst[i] = 0.0, k + 1
    return s


def rows_of(scan):
    """The rows of an AxisScan of tests/test_person_motion.py as row specs; its beam at max_range (20 m there) moves to
    MAX_RANGE."""
    out = []
    for k in range(scan.nd):
        pts = [(int(i) % 4, float(scan.ranges[i])) for i in np.flatnonzero(scan.inst == k + 1)]
        pts = [(a, MAX_RANGE if r == DEFAULTS["max_range"] else r) for a, r in pts]
        out.append((pts, float(scan.det_cls[k]), tuple(scan.det_xy[k])))
    return out


def embed(scans, at, N, points=2):
    """The scene ``scans`` (AxisScans, or lists of row specs) replayed from detection row ``at`` of N beams, behind
    the decoys 0..at-1.  -> list of AxisScan."""
    return [place(N, list(range(at)) + (rows_of(s) if isinstance(s, AxisScan) else list(s)), t, points)
            for t, s in enumerate(scans)]


def run(scans, **kw):
    """The restatement over placed scans.  -> (outputs, states) per scan."""
    return run_axis(scans, **kw)


def point_scans():
    """The rules of tests/test_person_motion.rule_scans and both ties with single-point rows on the axes (settings:
    KW1), 12 beams at most, three per axis.  -> three lists of row specs; POINT_PREV has what the second and third
    scan must give."""
    a = [pt(0, 1.0), pt(0, 3.0), pt(1, 2.0), pt(2, 4.0), pt(3, 5.0), pt(3, 8.0), pt(1, 10.25), pt(1, 9.75)]
    b = [pt(0, 3.75),                                          # 0: 0.75 m from a's row 1: the reach of the far variant
         pt(0, 1.125),                                         # 1: pairs with a's row 0
         ([], 0.9, (0.0, 0.0)),                                # 2: no points: under min_points = 1
         pt(1, 2.125, cls=0.2),                                # 3: below cls_thresh
         pt(2, 4.25), pt(2, 3.875),                            # 4, 5: both nearest to a's row 3; 5 is the mutual one
         pt(3, 5.25), pt(3, 4.75),                             # 6, 7: tie for a's row 4: the lower row
         ([(3, 8.125), (0, MAX_RANGE), (1, np.inf), (2, np.nan)], 0.9, (0.0, -8.125)),   # 8: three ranges left out
         pt(1, 10.0)]                                          # 9: a's rows 6 and 7 tie: the lower row
    c = [pt(1, 2.25),                                          # 0: next to b's row 3, which was not valid
         pt(0, 1.25)]                                          # 1: pairs with b's row 1
    return [a, b, c]


POINT_PREV = ([-1, 0, -1, -1, -1, 3, 4, -1, 5, 6], [-1, 1])    # det_prev of the scene's rows, before the shift by at
POINT_PREV_FAR = [1, 0, -1, -1, -1, 3, 4, -1, 5, 6]            # reach = 0.75
POINT_FLOW = {1: (0.125, 0.0), 5: (0.125, 0.0), 6: (0.0, -0.25), 8: (0.0, -0.125), 9: (0.0, -0.25)}
RULE_PREV = ([-1, 0, -1, -1, -1, 4, -1, 5], [-1, -1, 1])       # tests/test_person_motion.py's literals
RULE_PREV_FAR = [1, 0, -1, -1, -1, 4, -1, 5]
RULE_PREV_LOOSE = ([-1, 0, 2, 3, -1, 4, -1, 5], [2, 3, 1])


def gate_scans():
    """The two gates that compare with a setting, at equality and one step beside it (settings: KW1).
    -> three lists of row specs; GATE_PREV has the partners."""
    edge = ([(0, below32(MAX_RANGE)), (1, MAX_RANGE)], 0.9, (below32(MAX_RANGE), 0.0))
    a = [pt(2, 12.0, cls=0.5),                                 # 0: det_cls == cls_thresh: valid
         pt(3, 16.0, cls=below(0.5)),                          # 1: one step below: not valid
         edge,                                                 # 2: the range one float32 below max_range counts,
         pt(1, 20.0, cls=0.5)]                                 # 3     the one at max_range does not: det_count = 1
    b = [pt(2, 12.125, cls=0.5),                               # 0: pairs with a's row 0
         pt(3, 16.125),                                        # 1: a's row 1 was no candidate
         edge,                                                 # 2: pairs with a's row 2, flow 0
         pt(1, 20.125, cls=below(0.5))]                        # 3: not valid itself
    c = [pt(1, 20.25),                                         # 0: b's row 3 was no candidate
         pt(3, 16.25)]                                         # 1: pairs with b's row 1
    return [a, b, c]


GATE_PREV = ([0, -1, 2, -1], [-1, 1])

# (N, at) of the two-point scenes and of the single-point ones (see the module docstring)
PLACEMENTS2 = ((192, 60), (512, 64), (512, 120), (2048, 505), (4096, 512), (4096, 2030))
PLACEMENTS1 = ((128, 60), (512, 448), (512, 500), (1024, 505), (4096, 4084))
GATE_PLACEMENTS = ((128, 62), (512, 500), (1024, 510), (4096, 3582))


def boundary_tie(kind, N, lo, hi):
    """Two scans of hi + 1 rows, decoys but for the rows lo and hi.  "previous": the previous rows lo and hi are
    0.25 m either side of the current row lo.  "current": the current rows lo and hi are 0.25 m either side of the
    previous row lo.  Either way row lo pairs with row lo and row hi with nobody."""
    rows = lambda x, y: [x if k == lo else y if k == hi else k for k in range(hi + 1)]
    if kind == "previous":
        first, second = rows(xy_row(0.25, 0.0), xy_row(-0.25, 0.0)), rows(xy_row(0.0, 0.0), xy_row(8.0, 8.0))
    else:
        first, second = rows(xy_row(0.0, 0.0), xy_row(8.0, 8.0)), rows(xy_row(0.0, 0.25), xy_row(0.0, -0.25))
    return [place(N, first, 0), place(N, second, 1)]


BOUNDARY_TIES = ((256, 63, 64), (256, 64, 127), (1280, 511, 512), (1280, 63, 64))      # (N, lo, hi)


def mutual_scene(N, j, k_lo, k_hi):
    """The previous row j is the nearest of the current rows k_lo (0.25 m) and k_hi (0.125 m): k_hi has it."""
    first = [xy_row(-4.0, 1.0) if k == j else k for k in range(j + 1)]
    second = [xy_row(-4.25, 1.0) if k == k_lo else xy_row(-3.875, 1.0) if k == k_hi else k for k in range(k_hi + 1)]
    return [place(N, first, 0), place(N, second, 1)]


MUTUALS = ((256, 70, 10, 80), (2048, 600, 100, 700))           # (N, j, k_lo, k_hi)


def slot_count_scans(N, big, small):
    """big, small, big rows: decoy f is row f of the long scans and row big - 1 - f of the short one, which holds the
    decoys big - small .. big - 1.  So the short scan pairs with previous rows >= small, beyond its own num_det, and the
    last scan's rows >= small, beyond prev_num, pair with the previous rows below small."""
    return [place(N, list(range(big)), 0), place(N, [big - 1 - k for k in range(small)], 1),
            place(N, list(range(big)), 2)]


SLOT_COUNTS = ((512, 130, 60), (2560, 1030, 500))


def margins(scans, **kw):
    """-> (ties, smallest margin): over every scan after the first, every current candidate against every previous
    one and the reverse -- the gap between the two smallest d2 of a row or column, and every d2 against reach^2; a gap
    of 0 counts as a tie (equal doubles: equal bits, no d2 is -0), anything else goes into the margin."""
    outs, states = run(scans, **kw)
    reach2 = kw["reach"] ** 2
    ties, least = 0, np.inf
    for t in range(1, len(scans)):
        cur, prev = np.flatnonzero(states[t]["prev_cand"]), np.flatnonzero(states[t - 1]["prev_cand"][:int(states[t - 1]["prev_num"])])
        c, p = outs[t]["det_centre"][cur], states[t - 1]["prev_centre"][prev]
        if not len(cur) or not len(prev):
            continue
        for a, b in ((c, p), (p, c)):
            for lo in range(0, len(a), 256):
                dx, dy = a[lo:lo + 256, None, 0] - b[None, :, 0], a[lo:lo + 256, None, 1] - b[None, :, 1]
                d2 = dx * dx + dy * dy
                gate = np.abs(d2 - reach2)
                least = min(least, gate[gate > 0].min(initial=np.inf))
                if d2.shape[1] >= 2:
                    two = np.partition(d2, 1, axis=1)[:, :2]
                    gap = two[:, 1] - two[:, 0]
                    inside = two[:, 0] <= reach2               # a tie beyond the reach decides nothing
                    ties += int((inside & (gap == 0)).sum())
                    least = min(least, gap[gap > 0].min(initial=np.inf))
    return ties, least


def check_embedded(scans, at, N, source, want, flows=None, **kw):
    """What every embedded scene must give, from the restatement alone: the partners shifted by ``at``, the scene's
    det_flow as ``source`` (the same scene at row 0 of a short scan) has it, every decoy paired with itself."""
    outs, _ = run(scans, **kw)
    plain, _ = run(source, **kw)
    for t in (1, 2):
        n = len(want[t - 1])
        shifted = [j + at if j >= 0 else -1 for j in want[t - 1]]
        assert list(outs[t]["det_prev"][at:at + n]) == shifted, (N, at, t)
        assert same_bits(outs[t]["det_flow"][at:at + n], plain[t]["det_flow"][:n]), (N, at, t)
        assert np.array_equal(outs[t]["det_prev"][:at], np.arange(at)), (N, at, t)
        assert np.array_equal(outs[t]["det_flow"][:at], 0.125 * np.array([AXES[f % 4] for f in range(at)]).reshape(-1, 2))
        for k, f in (flows or {}).items():
            if t == 1:
                assert np.array_equal(outs[t]["det_flow"][at + k], f), (N, at, k)
    return outs


# ---- the tests of section 1
@pytest.mark.parametrize("N,at", PLACEMENTS2)
def test_two_point_scenes_keep_their_answers_behind_the_decoys(N, at):
    outs = check_embedded(embed(rule_scans(), at, N), at, N, embed(rule_scans(), 0, 64), RULE_PREV, **KW2)
    o = outs[1]
    # a pair, and one refused row of each kind: beyond reach, one point, below the threshold, not mutual, no points
    assert o["det_prev"][at + 1] == at and list(o["det_count"][at:at + 8]) == [2, 2, 1, 2, 2, 2, 0, 2]
    assert list(o["det_valid"][at:at + 8]) == [1, 1, 1, 0, 1, 1, 1, 1] and np.isnan(o["det_centre"][at + 6]).all()
    far = run(embed(rule_scans(), at, N), **dict(KW2, reach=0.75))[0][1]
    assert list(far["det_prev"][at:at + 8]) == [j + at if j >= 0 else -1 for j in RULE_PREV_FAR]
    assert np.array_equal(far["det_flow"][at], [0.75, 0.0])                    # d2 = 0.5625 = reach^2 exactly
    check_embedded(embed(rule_scans(), at, N), at, N, embed(rule_scans(), 0, 64), RULE_PREV_LOOSE,
                   **dict(KW2, min_points=1, cls_thresh=0.1))
    ties = tie_scans()
    o = run(embed(ties["previous rows"], at, N), **KW2)[0][1]
    assert o["det_prev"][at] == at + 1 and np.array_equal(o["det_flow"][at], [-0.25, 0.0])
    o = run(embed(ties["current rows"], at, N), **KW2)[0][1]
    assert list(o["det_prev"][at:at + 3]) == [-1, at, -1] and np.array_equal(o["det_flow"][at + 1], [0.0, 0.25])
    assert owner(at + 7, N)[1] >= 1


@pytest.mark.parametrize("N,at", PLACEMENTS1)
def test_single_point_scene_keeps_its_answers_behind_the_decoys(N, at):
    outs = check_embedded(embed(point_scans(), at, N, 1), at, N, embed(point_scans(), 0, 64, 1), POINT_PREV, POINT_FLOW,
                          **KW1)
    o = outs[1]
    assert list(o["det_count"][at:at + 10]) == [1, 1, 0, 1, 1, 1, 1, 1, 1, 1]
    assert list(o["det_valid"][at:at + 10]) == [1, 1, 1, 0, 1, 1, 1, 1, 1, 1] and np.isnan(o["det_centre"][at + 2]).all()
    far = run(embed(point_scans(), at, N, 1), **dict(KW1, reach=0.75))[0][1]
    assert list(far["det_prev"][at:at + 10]) == [j + at if j >= 0 else -1 for j in POINT_PREV_FAR]
    assert np.array_equal(far["det_flow"][at], [0.75, 0.0])
    assert owner(at + 9, N)[1] >= 1


def test_the_placements_reach_the_slots_lanes_and_waves_they_are_for():
    """(thread, slot, wave) of the scene's first and last deciding row, as the launcher lays the rows out."""
    first = {(N, at): owner(at, N) for N, at in PLACEMENTS2 + PLACEMENTS1}
    last = {(N, at): owner(at + (7 if (N, at) in PLACEMENTS2 else 9), N) for N, at in PLACEMENTS2 + PLACEMENTS1}
    assert first[192, 60] == (60, 0, 0) and last[192, 60] == (3, 1, 0)          # straddles the lanes 60..63 | 0..3
    assert first[128, 60] == (60, 0, 0) and last[128, 60] == (5, 1, 0)          # the smallest shape with a second slot
    assert first[512, 64] == (0, 1, 0) and first[512, 120] == (56, 1, 0) and last[512, 120] == (63, 1, 0)
    assert first[512, 448] == (0, 7, 0) and last[512, 500] == (61, 7, 0)        # the wave form's last slot
    assert first[1024, 505] == (505, 0, 7) and last[1024, 505] == (2, 1, 0)     # rows 511 | 512 of the group form
    assert first[2048, 505] == (505, 0, 7) and last[2048, 505] == (0, 1, 0)
    assert first[4096, 512] == (0, 1, 0) and first[4096, 2030] == (494, 3, 7) and last[4096, 2030] == (501, 3, 7)
    assert first[4096, 4084] == (500, 7, 7) and last[4096, 4084] == (509, 7, 7)  # the group form's last slot
    for N, at in GATE_PLACEMENTS:
        assert owner(at + 3, N)[1] >= 1                        # in, or across the boundary into, a later slot
    assert [owner(k, 128) for k in (62, 63, 64, 65)] == [(62, 0, 0), (63, 0, 0), (0, 1, 0), (1, 1, 0)]
    assert [owner(k, 512) for k in (500, 503)] == [(52, 7, 0), (55, 7, 0)]
    assert [owner(k, 1024)[1] for k in (510, 511, 512, 513)] == [0, 0, 1, 1]
    assert [owner(k, 4096) for k in (3582, 3583, 3584, 3585)] == [(510, 6, 7), (511, 6, 7), (0, 7, 0), (1, 7, 0)]
    for N, lo, hi in BOUNDARY_TIES:
        assert owner(lo, N)[:2] != owner(hi, N)[:2]
    assert (owner(63, 256), owner(64, 256), owner(127, 256)) == ((63, 0, 0), (0, 1, 0), (63, 1, 0))
    assert (owner(511, 1280), owner(512, 1280)) == ((511, 0, 7), (0, 1, 0))
    assert (owner(63, 1280), owner(64, 1280)) == ((63, 0, 0), (64, 0, 1))       # two waves of one slot
    for N, j, k_lo, k_hi in MUTUALS:
        assert (owner(j, N)[1], owner(k_lo, N)[1], owner(k_hi, N)[1]) == (1, 0, 1)


@pytest.mark.parametrize("N,at", GATE_PLACEMENTS)
def test_threshold_and_max_range_at_equality(N, at):
    scans = embed(gate_scans(), at, N, 1)
    outs = check_embedded(scans, at, N, embed(gate_scans(), 0, 64, 1), GATE_PREV, **KW1)
    assert list(outs[0]["det_valid"][at:at + 4]) == [1, 0, 1, 1] and list(outs[1]["det_valid"][at:at + 4]) == [1, 1, 1, 0]
    assert list(outs[1]["det_count"][at:at + 4]) == [1, 1, 1, 1]                # row 2: one of its two ranges counts
    assert np.array_equal(outs[1]["det_centre"][at + 2], [MAX_RANGE - 0.0625, 0.0])
    assert np.array_equal(outs[1]["det_flow"][at + 2], [0.0, 0.0]) and np.isnan(outs[1]["det_flow"][at + 1]).all()
    assert np.float32(below32(MAX_RANGE)) < np.float32(MAX_RANGE) and below(0.5) < 0.5


@pytest.mark.parametrize("N,lo,hi", BOUNDARY_TIES)
def test_ties_across_an_ownership_boundary_go_to_the_lower_row(N, lo, hi):
    for kind in ("previous", "current"):
        scans = boundary_tie(kind, N, lo, hi)
        o = run(scans, **KW2)[0][1]
        want = np.arange(hi + 1)
        want[hi] = -1
        assert np.array_equal(o["det_prev"][:hi + 1], want), (kind, N, lo, hi)
        assert np.array_equal(o["det_flow"][lo], [-0.25, 0.0] if kind == "previous" else [0.0, 0.25])
        ties, least = margins(scans, **KW2)
        assert ties >= 1 and least >= MARGIN


@pytest.mark.parametrize("N,j,k_lo,k_hi", MUTUALS)
def test_mutual_rule_between_slots(N, j, k_lo, k_hi):
    o = run(mutual_scene(N, j, k_lo, k_hi), **KW2)[0][1]
    assert o["det_prev"][k_hi] == j and o["det_prev"][k_lo] == -1 and np.array_equal(o["det_flow"][k_hi], [0.125, 0.0])
    others = np.array([k for k in range(j) if k != k_lo])
    assert np.array_equal(o["det_prev"][others], others) and (o["det_prev"][j:k_hi] == -1).all()


@pytest.mark.parametrize("N,big,small", SLOT_COUNTS)
def test_scans_of_different_slot_counts(N, big, small):
    T = threads_of(N)
    assert -(-big // T) > -(-small // T) >= 1                  # the slot counts differ
    outs, states = run(slot_count_scans(N, big, small), **KW2)
    assert [int(s["prev_num"]) for s in states] == [big, small, big]
    assert np.array_equal(outs[1]["det_prev"][:small], big - 1 - np.arange(small)) and (outs[1]["det_prev"][small:] == -1).all()
    assert outs[1]["det_prev"][:small].min() >= small          # every partner lies beyond this scan's num_det
    want = np.where(np.arange(big) >= big - small, big - 1 - np.arange(big), -1)
    assert np.array_equal(outs[2]["det_prev"][:big], want) and (want[small:] >= 0).sum() >= big - 2 * small > 0
    assert np.array_equal(outs[2]["det_flow"][big - 1], 0.125 * np.array(AXES[(big - 1) % 4]))


def test_no_decision_of_the_scenes_rests_on_rounding():
    """As tests/test_tracks.test_no_decision_of_the_scenario_rests_on_rounding: ties are counted, everything else has
    a margin; the largest placement of either row kind, the ties and the gates."""
    seen = []
    for scans, kw, ties_wanted in ((embed(rule_scans(), 2030, 4096), KW2, 0), (embed(rule_scans(), 60, 192), dict(KW2, reach=0.75), 0),
                                   (embed(point_scans(), 4084, 4096, 1), KW1, 2), (embed(point_scans(), 60, 128, 1), dict(KW1, reach=0.75), 2),
                                   (embed(tie_scans()["previous rows"], 512, 4096), KW2, 1),
                                   (embed(tie_scans()["current rows"], 64, 512), KW2, 1),
                                   (embed(gate_scans(), 510, 1024, 1), KW1, 0), (slot_count_scans(512, 130, 60), KW2, 0),
                                   (mutual_scene(256, 70, 10, 80), KW2, 0)):
        ties, least = margins(scans, **kw)
        seen.append((ties, least))
        assert ties == ties_wanted and least >= MARGIN, (ties, least)
    print("ties and smallest margins:", seen)


# ---------------------------------------------------------------- 2. tracker scenes
def far_rows(n, x0=-1000.0, y0=-1000.0):
    """n centres 8 m apart, far from everything."""
    return np.stack([x0 - 8.0 * np.arange(n), np.full(n, y0)], axis=1)


def births(M, placed):
    """A first scan of M rows, row s -> slot s: ``placed`` {slot: (x, y)}, the others 8 m apart and far away."""
    xy = far_rows(M, 1000.0, 500.0)
    for s, p in placed.items():
        xy[s] = p
    return xy


def second_scan(N, placed, rows=None):
    """A scan of ``rows`` valid rows (default: up to the last placed one), far away but for ``placed`` {row: (x, y)}."""
    n = max(placed) + 1 if rows is None else rows
    xy = far_rows(n)
    for k, p in placed.items():
        xy[k] = p
    return scan_of(xy, N=N)


CHAIN = dict(A=70, B=(3, 20, 100))                             # slot 70: lane 6, second register slot; lanes 3, 20, 36
CHAIN_TRACKS = {70: (0.0, 0.0), 3: (0.625, 0.0), 20: (0.0, 1.0), 100: (-1.375, 0.0)}
CHAIN_CANDS = ((0.5, 0.0), (0.0, 0.75), (-1.0, 0.0), (0.0, -1.25))     # A's first .. fourth choice; B1..B3 are nearer


def chain_rows(N):
    """The rows of A's four choices: in reverse row order at N = 128, behind row 1024 at the long scans (the last
    one in the third staged chunk at N = 2049)."""
    return (3, 2, 1, 0) if N == 128 else (1100, 1500, N - 1, 1030)


def track_scenes():
    """-> {name: (M, N, seq, settings, expect)}: expect = {field: {index: value}} of the last state, on top of the
    comparison with track_step.  Births from a first scan, zero flows: every prediction is exact."""
    K = dict(SETTINGS, gate=2.5)
    sc = {}
    for N in (128, 2048, 2049):
        row = 0 if N == 128 else N - 1
        sc["same lane/%d" % N] = (66, N, [scan_of(births(66, {1: (-0.25, 0.0), 65: (0.25, 0.0)}), N=N),
                                          second_scan(N, {row: (0.0, 0.0)})], K,
                                  dict(track_det={1: row, 65: -1}, track_misses={1: 0, 65: 1}))
        rows = chain_rows(N)
        for last in (4, 3):
            placed = {rows[i]: CHAIN_CANDS[i] for i in range(last)}
            want = dict(track_det={3: rows[0], 20: rows[1], 100: rows[2], 70: rows[3] if last == 4 else -1},
                        track_misses={70: 0 if last == 4 else 1})
            sc["chain %d/%d" % (last, N)] = (128, N, [scan_of(births(128, CHAIN_TRACKS), N=N), second_scan(N, placed)], K, want)
    four = {2: (-0.25, 0.0), 66: (0.25, 0.0), 130: (0.0, -0.25), 194: (0.0, 0.25)}
    sc["same lane, four slots"] = (256, 256, [scan_of(births(256, four), N=256), second_scan(256, {0: (0.0, 0.0)})], K,
                                   dict(track_det={2: 0, 66: -1, 130: -1, 194: -1}, track_misses={2: 0, 66: 1, 130: 1, 194: 1}))
    half = dict(SETTINGS, gate=0.5)
    one = lambda p: [scan_of([[0.0, 0.0]], N=4), scan_of([p], N=4)]
    sc["gate, at it"] = (4, 4, one([0.5, 0.0]), half, dict(track_det={0: 0}, track_id={1: 0}, next_id={(): 2}))
    sc["gate, beyond"] = (4, 4, one([float(np.nextafter(0.5, 1.0)), 0.0]), half,
                          dict(track_det={0: -1, 1: 0}, track_misses={0: 1}, track_id={0: 1, 1: 2}, next_id={(): 3}))
    zero = dict(SETTINGS, gate=0.0)
    sc["gate 0, on it"] = (4, 4, one([0.0, 0.0]), zero, dict(track_det={0: 0}, next_id={(): 2}))
    sc["gate 0, beside"] = (4, 4, one([2.0 ** -500, 0.0]), zero, dict(track_det={0: -1, 1: 0}, track_id={0: 1, 1: 2}))
    # the same gate in the second register slot of lane 6
    at70 = lambda p: [scan_of(births(128, {70: (0.0, 0.0)}), N=128), second_scan(128, {5: p})]
    sc["gate, at it, slot 70"] = (128, 128, at70((0.0, -0.5)), half, dict(track_det={70: 5}, track_misses={70: 0}))
    sc["gate, beyond, slot 70"] = (128, 128, at70((0.0, -float(np.nextafter(0.5, 1.0)))), half,
                                   dict(track_det={70: -1}, track_misses={70: 1}))
    # the per-step lists are slot 0's: freed at misses = max_misses + 1 and not before; the birth reuses the slot at once
    sc["max_misses 0"] = (1, 4, one([5.0, 5.0]), dict(SETTINGS, max_misses=0),
                          dict(track_id={0: 2}, dropped={(): 0}, track_misses={0: 0}, track_det={0: 0},
                               steps=dict(track_id=[1, 2], dropped=[0, 0])))
    sc["max_misses 1"] = (1, 4, one([5.0, 5.0]) + [scan_of([[5.0, 5.0]], N=4)], dict(SETTINGS, max_misses=1),
                          dict(track_id={0: 2}, track_det={0: 0},
                               steps=dict(track_id=[1, 1, 2], dropped=[0, 1, 0], track_misses=[0, 1, 0])))
    others = np.delete(births(128, {}), 70, axis=0)            # everyone but slot 70 is seen again
    sc["max_misses 1, slot 70"] = (128, 128, [scan_of(births(128, {}), N=128), scan_of(others, N=128)],
                                   dict(SETTINGS, max_misses=1),
                                   dict(track_id={70: 71, 69: 70}, track_misses={70: 1, 69: 0, 71: 0}, track_det={70: -1, 71: 70}))
    for hits in (0, 1, 2):
        sc["min_hits %d" % hits] = (4, 4, [scan_of([[0.0, 0.0]], N=4)], dict(SETTINGS, min_hits=hits),
                                    dict(track_confirmed={0: int(hits <= 1), 1: 0}))
    return sc


def check_expectations(state, expect, what, steps=None):
    """``state``: the last state of one sensor; ``steps``: slot 0 (or the scalar) of every field after every step."""
    for field, values in expect.get("steps", {}).items():
        if steps is not None:
            assert [int(np.asarray(st[field]).reshape(-1)[0]) for st in steps] == values, (what, field)
    for field, items in expect.items():
        if field == "steps":
            continue
        for index, value in items.items():
            assert int(state[field][index]) == value, (what, field, index, int(state[field][index]), value)


def greedy_order(tracks, cands, gate):
    """The (slot, candidate) pairs in the order the greedy rounds take them: a guard on the chain scene's geometry,
    not a referee -- track_step decides what the answer is."""
    slots, rows = sorted(tracks), sorted(cands)
    cost = np.array([[(cands[k][0] - tracks[s][0]) ** 2 + (cands[k][1] - tracks[s][1]) ** 2 for k in rows] for s in slots])
    cost = np.where(cost <= gate * gate, cost, np.inf)
    order = []
    while np.isfinite(cost).any():
        i, j = np.unravel_index(np.argmin(cost), cost.shape)
        order.append((slots[i], rows[j]))
        cost[i, :] = cost[:, j] = np.inf
    return order


def test_tracker_scenes_give_the_stated_answers():
    for name, (M, N, seq, kw, expect) in track_scenes().items():
        gaps = []
        states = run_steps(seq, M, N, margins=gaps, **kw)
        check_expectations(states[-1], expect, name, steps=states)
        pair = [m for kind, m in gaps if kind == "pair"]
        if name.startswith("chain"):
            assert pair and min(pair) >= MARGIN, (name, pair)  # no round of the chain is a tie
        if name.startswith("same lane"):
            assert 0.0 in pair                                 # the tie is one of equal bits


@pytest.mark.parametrize("N", [128, 2048, 2049])
def test_chain_takes_the_k_th_choice_of_a_in_round_k(N):
    rows = chain_rows(N)
    A, (B1, B2, B3) = CHAIN["A"], CHAIN["B"]
    assert (A % 64, A // 64) == (6, 1) and all(b % 64 != 6 for b in CHAIN["B"])
    cost = [(x - CHAIN_TRACKS[A][0]) ** 2 + (y - CHAIN_TRACKS[A][1]) ** 2 for x, y in CHAIN_CANDS]
    assert cost == sorted(cost) and len(set(cost)) == 4 and cost[3] <= 2.5 ** 2      # A's order of choice, all inside
    cands = {rows[i]: CHAIN_CANDS[i] for i in range(4)}
    assert greedy_order(CHAIN_TRACKS, cands, 2.5) == [(B1, rows[0]), (B2, rows[1]), (B3, rows[2]), (A, rows[3])]
    del cands[rows[3]]
    assert greedy_order(CHAIN_TRACKS, cands, 2.5) == [(B1, rows[0]), (B2, rows[1]), (B3, rows[2])]
    if N > 128:                                                # candidate = row here: the second and third chunk of 1024
        assert min(rows) >= 1024 and (max(rows) >= 2048) == (N == 2049)
        M_, N_, seq, _, _ = track_scenes()["chain 4/%d" % N]
        assert seq[1]["valid"][:N].all() and int(seq[1]["num_det"]) == N


# ---------------------------------------------------------------- 3. ego-motion base weights at equality
def ego_equality_case(N):
    """A rigid field of N points with the gates of the base weight planted at equality.  -> dict of the inputs of
    ops.ego_motion (xy, flow, ranges, weight, inst, num, det_cls; max_range 20, cls_thresh 0.5), ``at`` = the planted
    indices by name and ``counted`` = whether each counts."""
    rng = np.random.default_rng(N)
    xy = rng.normal(0.0, 5.0, (N, 2))
    flow = rigid_field(xy, 0.02, (0.04, -0.03))
    where = list(range(7)) if N == 8 else [512, 3, 64, 65, 511, 200, 450]
    names = ("at max_range", "below max_range", "at cls_thresh", "below cls_thresh", "tiny weight", "-0 weight", "0 weight")
    at = dict(zip(names, where))
    ranges, weight = np.ones(N, np.float32), np.ones(N, np.float32)
    ranges[at["at max_range"]] = 20.0
    ranges[at["below max_range"]] = np.nextafter(np.float32(20.0), np.float32(0.0))
    inst, det_cls = np.zeros(N, np.int32), np.zeros(N)
    inst[at["at cls_thresh"]], inst[at["below cls_thresh"]] = 1, 2
    det_cls[:2] = 0.5, below(0.5)
    weight[at["tiny weight"]], weight[at["-0 weight"]], weight[at["0 weight"]] = 2.0 ** -149, -0.0, 0.0
    counted = dict(zip(names, (False, True, False, True, True, False, False)))
    return dict(xy=xy, flow=flow, ranges=ranges, weight=weight, inst=inst, num=np.int32(2), det_cls=det_cls, at=at,
                counted=counted)


@pytest.mark.parametrize("N", [8, 513])
def test_ego_base_weights_at_equality(N):
    c = ego_equality_case(N)
    w0 = base_weights(c["xy"], c["flow"], weight=c["weight"], ranges=c["ranges"], inst=c["inst"], num=c["num"],
                      det_cls=c["det_cls"])
    for name, i in c["at"].items():
        assert (w0[i] > 0) == c["counted"][name], name
    assert int((w0 > 0).sum()) == N - 4 and w0[c["at"]["tiny weight"]] == 2.0 ** -149 and w0.astype(np.float32)[c["at"]["tiny weight"]] > 0


# ---------------------------------------------------------------- the builders themselves
def test_builders_state_what_they_build():
    s = place(64, [0, 1, xy_row(1.0, -2.0), 5], t=2)
    assert s.nd == 4 and list(np.bincount(s.inst, minlength=5)) == [56, 2, 2, 2, 2]
    o = s.step(motion_state(64), max_range=MAX_RANGE)
    assert np.array_equal(o["det_centre"][:4], [[64.25, 0], [0, 64.25], [1, -2], [0, 66.25]]) and list(o["det_count"][:4]) == [2] * 4
    with pytest.raises(IndexError):
        embed(rule_scans(), 60, 128)                           # 2 x 60 + 16 beams: the reason for (192, 60)
    with pytest.raises(IndexError):
        embed(point_scans(), 501, 512, 1)
    a, b, c = (embed(rule_scans(), 0, 64)[t] for t in range(3))
    for mine, theirs in zip((a, b, c), rule_scans()):          # at row 0 of 64 beams: the scene itself, but for the
        assert mine.nd == theirs.nd and np.array_equal(mine.det_xy, theirs.det_xy)     # moved max_range beam
        assert np.array_equal(mine.inst, theirs.inst)
    assert same_bits(run([a, b, c], **KW2)[0][1]["det_flow"], run_axis(rule_scans())[0][1]["det_flow"])
