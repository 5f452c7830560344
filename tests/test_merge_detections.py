"""Merged detections (pof_merge_detections, N18) without a GPU: ``merge_detections_oracle`` is the NumPy restatement of
the comment in include/pof_abi.h -- one sensor, one walk over B's rows -- checked here rule by rule on scenes held to
literal values, on seeded patterns for the shapes the device runs, and on rooms with people for what the merge is good
for.  tests/test_merge_detections_gpu.py imports the restatement and the scenes and holds the device to them bit for
bit: the stage is integers and bitwise copies, so there is no tolerance anywhere.

Rule scenes.  N = 8 unless the name says otherwise; scores are dyadic (0.75 confident, 0.25 not, at cls_thresh 0.5).  B
row k has the centre ``BXY[k]`` and the score 1.0, A row j the centre ``AXY[j]``.  ``FLIPS`` names, per rule, the scene
in which the restatement with that rule turned round gives another output; the same turns in the kernel fail
tests/test_merge_detections_gpu.py::test_rule_scenes at that scene."""
import inspect
import os
import re

import numpy as np
import pytest

from test_grid_cast import grid_cast_oracle
from test_grid_map import grid_map_oracle
from test_novel_segments import novel_segments_oracle, same_bits
from test_person_motion import motion_state, people_scene, person_motion_oracle, same_bits as same_bits_nan
from test_tracks import FLOAT_FIELDS as TRACK_FLOAT, INT_FIELDS as TRACK_INT, new_state as new_track_state, track_step

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = dict(cls_thresh=0.5, absorb_pct=50)
OUT_FIELDS = ("instance_mask", "num_det", "det_xy", "det_cls", "det_points", "det_src", "det_row", "b_row", "b_count",
              "b_known", "merge_count")
OUT_DTYPES = (np.int32, np.int32, np.float64, np.float64, np.int32, np.uint8, np.int32, np.int32, np.int32, np.int32,
              np.int32)
NAN = np.nan


def _clamp(n, N):
    return min(max(int(n), 0), N)


# ---------------------------------------------------------------- restatement of the device rule, one sensor
def merge_detections_oracle(b_inst, b_num, b_xy, b_cls, a_inst=None, a_num=None, a_xy=None, a_cls=None, cls_thresh=0.5,
                            absorb_pct=50, flip=None):
    """One scan of one sensor.  b_inst [N], b_num, b_xy [N,2], b_cls [N]: the secondary record; a_*: the primary record,
    all four or none.  ``flip``: one rule of the header turned round, for ``FLIPS``.  -> dict of the eleven outputs."""
    b_ids = np.asarray(b_inst, np.int64)
    N = len(b_ids)
    nB = _clamp(b_num, N)
    nA = 0 if a_inst is None else _clamp(a_num, N)
    a_ids = np.zeros(N, np.int64) if a_inst is None else np.asarray(a_inst, np.int64)
    a_own = (a_ids >= 1) & (a_ids <= nA)
    confident = np.zeros(N, bool)
    if a_inst is not None:
        score = np.asarray(a_cls, np.float64)[np.where(a_own, a_ids - 1, 0)]
        with np.errstate(invalid="ignore"):
            confident = a_own & (score > cls_thresh if flip == "confident >" else score >= cls_thresh)
    member = (b_ids >= 1) & (b_ids <= nB)
    b_count = np.bincount(b_ids[member] - 1, minlength=N).astype(np.int32)
    b_known = np.bincount(b_ids[member & confident] - 1, minlength=N).astype(np.int32)
    R = N + 1                                                  # one spare row: the flipped capacity cut writes it
    xy, cls = np.zeros((R, 2)), np.zeros(R)
    src, from_row = np.zeros(R, np.uint8), np.zeros(R, np.int32)
    b_row = np.full(N, -1, np.int32)
    mask = np.where(a_own, a_ids, 0)
    if nA:
        xy[:nA], cls[:nA] = np.asarray(a_xy, np.float64)[:nA], np.asarray(a_cls, np.float64)[:nA]
        src[:nA], from_row[:nA] = 1, np.arange(nA)
    rows = nA
    absorbed = dropped = 0
    for k in range(nB):                                        # the one walk over B's rows
        count, known = int(b_count[k]), int(b_known[k])
        empty = count == 0 and flip != "empty kept"
        if flip == "absorb >":
            full = 100 * known > absorb_pct * count
        else:
            full = 100 * known >= absorb_pct * count
        if empty or (full and count != 0):
            absorbed += 1
            continue
        if not (rows <= N if flip == "capacity <=" else rows < N):
            b_row[k] = -2
            dropped += 1
            continue
        b_row[k] = rows
        xy[rows], cls[rows] = np.asarray(b_xy, np.float64)[k], np.asarray(b_cls, np.float64)[k]
        src[rows], from_row[rows] = 2, k
        takes = (b_ids == k + 1) & member
        if flip != "takes confident":
            takes &= ~confident
        mask[takes] = rows + 1
        rows += 1
    points = np.bincount(mask[mask > 0] - 1, minlength=R).astype(np.int32)
    return dict(instance_mask=mask.astype(np.int32), num_det=np.int32(rows), det_xy=xy[:N], det_cls=cls[:N],
                det_points=points[:N], det_src=src[:N], det_row=from_row[:N], b_row=b_row, b_count=b_count,
                b_known=b_known, merge_count=np.array([nA, rows - nA, absorbed, dropped], np.int32))


def run_case(case, flip=None):
    """The restatement on a case: dict(b=(inst, num, xy, cls), a=the same four or None, kw)."""
    return merge_detections_oracle(*case["b"], *(case["a"] or ()), flip=flip, **case["kw"])


# ---------------------------------------------------------------- rule scenes: literal values
HALF_DOWN = float(np.nextafter(0.5, 0.0))
NAN_PAYLOAD = float(np.array([0x7FF8000000000123], np.uint64).view(np.float64)[0])
BXY = [[10.0 + k, -(10.0 + k)] for k in range(8)]
AXY = [[0.25 * (j + 1), -0.5 * (j + 1)] for j in range(8)]
Z8 = [0] * 8
ZXY = [0.0, 0.0]


def _scene(b_inst, b_num, a_inst=None, a_num=None, a_cls=None, a_xy=None, b_cls=None, **kw):
    n = len(b_inst)
    b = (np.asarray(b_inst, np.int32), np.int32(b_num), np.asarray(BXY[:n], np.float64),
         np.asarray([1.0] * n if b_cls is None else b_cls, np.float64))
    a = None
    if a_inst is not None:
        a_cls = list(a_cls) + [0.0] * (n - len(a_cls))
        a = (np.asarray(a_inst, np.int32), np.int32(a_num), np.asarray(AXY[:n] if a_xy is None else a_xy, np.float64),
             np.asarray(a_cls, np.float64))
    return dict(b=b, a=a, kw=dict(DEFAULTS, **kw))


# a confident A row on the points 0, 1 and 4; B row 0 holds the points 0-3 (2 of 4 known), B row 1 the points 4-7 (1 of 4)
HALVES = dict(b_inst=[1, 1, 1, 1, 2, 2, 2, 2], b_num=2, a_inst=[1, 1, 0, 0, 1, 0, 0, 0], a_num=1, a_cls=[0.75])
INSIDE = dict(b_inst=[0, 0, 1, 1, 1, 0, 0, 0], b_num=1, a_inst=[0, 1, 1, 1, 1, 1, 1, 0], a_num=1, a_cls=[0.75])
NO_A = dict(b_inst=[1, 1, 1, 0, 2, 2, 0, 3], b_num=3)
AXY_ODD = [[-0.0, NAN_PAYLOAD], [0.0, -0.0], [NAN, 3.0]] + AXY[3:]


def rule_scenes():
    """-> {name: case}; EXPECTED says what each gives."""
    return {
        "nB 0": _scene([1, 1, 2, 2, 0, 0, 0, 0], 0, [1, 1, 1, 0, 2, 2, 0, 0], 2, [0.75, 0.25]),
        "A absent": _scene(**NO_A),
        "inside a confident row": _scene(**INSIDE),
        "2 of 4 and 1 of 4": _scene(**HALVES),
        "absorb_pct 24": _scene(absorb_pct=24, **HALVES),
        "absorb_pct 25": _scene(absorb_pct=25, **HALVES),      # 100 * 1 == 25 * 4
        "absorb_pct 26": _scene(absorb_pct=26, **HALVES),
        "over an unconfident row": _scene([0, 0, 1, 1, 0, 0, 0, 0], 1, [0, 1, 1, 1, 1, 0, 0, 0], 1, [0.25]),
        "every point of an unconfident row": _scene([0, 1, 1, 1, 0, 0, 0, 0], 1, [0, 1, 1, 0, 0, 0, 0, 0], 1, [0.25]),
        # scores at cls_thresh, the float64 below it and NaN; A's centres hold negative zeros and NaN payloads
        "score borders": _scene([1, 1, 2, 2, 3, 3, 0, 0], 3, [1, 1, 2, 2, 3, 3, 0, 0], 3, [0.5, HALF_DOWN, NAN_PAYLOAD],
                                a_xy=AXY_ODD, b_cls=[1.0, -0.0, NAN_PAYLOAD, 0.0, 0.0, 0.0, 0.0, 0.0]),
        "absorb_pct 0": _scene(absorb_pct=0, **NO_A),
        "absorb_pct 101": _scene(absorb_pct=101, **INSIDE),
        "B ids": _scene([0, 3, -1, 1, 1, 2, 2, -7], 2),
        "A ids": _scene([1, 1, 1, 0, 0, 0, 0, 0], 1, [0, 3, -1, 1, 1, 2, 2, -5], 2, [0.75, 0.75, 0.75]),
        # both counts are 8 then: id 8 is row 7, id 9 is nobody's; row 7 of B is 1 of 2 known
        "num_det beyond N": _scene([8, 8, 9, 0, 0, 0, 0, 0], 100, [8, 9, 0, 0, 0, 0, 0, 0], 100, [0.25] * 7 + [0.75]),
        "num_det below 0": _scene([1, 1, 2, 2, 0, 0, 0, 0], -1, [1, 1, 1, 0, 2, 2, 0, 0], -3, [0.75, 0.75]),
        "empty row between": _scene([1, 1, 0, 0, 3, 3, 0, 0], 3),
        "ranks": _scene([1, 1, 2, 2, 3, 3, 0, 0], 3, [0, 0, 1, 1, 0, 0, 0, 0], 1, [0.75]),
        "nA N - 1": _scene([1, 1, 2, 2, 0, 0, 0, 0], 2, Z8, 7, [0.75] * 7),
        "nA N": _scene([1, 1, 2, 2, 0, 0, 0, 0], 2, [0, 0, 0, 0, 5, 5, 0, 0], 8, [0.25] * 8),
        "N 1": _scene([1], 1),
        "N 1 with A": _scene([1], 1, [1], 1, [0.75]),
    }


def _rows(*rows, n=8, fill=0):
    return list(rows) + [fill] * (n - len(rows))


HALVES_KEPT = dict(instance_mask=[1, 1, 0, 0, 1, 2, 2, 2], num_det=2, det_xy=_rows(AXY[0], BXY[1], fill=ZXY),
                   det_cls=_rows(0.75, 1.0, fill=0.0), det_points=_rows(3, 3), det_src=_rows(1, 2), det_row=_rows(0, 1),
                   b_row=_rows(-1, 1, fill=-1), b_count=_rows(4, 4), b_known=_rows(2, 1), merge_count=[1, 1, 1, 0])
HALVES_GONE = dict(instance_mask=[1, 1, 0, 0, 1, 0, 0, 0], num_det=1, det_xy=_rows(AXY[0], fill=ZXY),
                   det_cls=_rows(0.75, fill=0.0), det_points=_rows(3), det_src=_rows(1), det_row=Z8, b_row=[-1] * 8,
                   b_count=_rows(4, 4), b_known=_rows(2, 1), merge_count=[1, 0, 2, 0])
# per scene the literal value of every field named, whole
EXPECTED = {
    "nB 0": dict(instance_mask=[1, 1, 1, 0, 2, 2, 0, 0], num_det=2, det_xy=_rows(AXY[0], AXY[1], fill=ZXY),
                 det_cls=_rows(0.75, 0.25, fill=0.0), det_points=_rows(3, 2), det_src=_rows(1, 1), det_row=_rows(0, 1),
                 b_row=[-1] * 8, b_count=Z8, b_known=Z8, merge_count=[2, 0, 0, 0]),
    "A absent": dict(instance_mask=[1, 1, 1, 0, 2, 2, 0, 3], num_det=3, det_xy=_rows(*BXY[:3], fill=ZXY),
                     det_cls=_rows(1.0, 1.0, 1.0, fill=0.0), det_points=_rows(3, 2, 1), det_src=_rows(2, 2, 2),
                     det_row=_rows(0, 1, 2), b_row=_rows(0, 1, 2, fill=-1), b_count=_rows(3, 2, 1), b_known=Z8,
                     merge_count=[0, 3, 0, 0]),
    "inside a confident row": dict(instance_mask=[0, 1, 1, 1, 1, 1, 1, 0], num_det=1, det_xy=_rows(AXY[0], fill=ZXY),
                                   det_cls=_rows(0.75, fill=0.0), det_points=_rows(6), det_src=_rows(1), det_row=Z8,
                                   b_row=[-1] * 8, b_count=_rows(3), b_known=_rows(3), merge_count=[1, 0, 1, 0]),
    "2 of 4 and 1 of 4": HALVES_KEPT,
    "absorb_pct 24": HALVES_GONE,
    "absorb_pct 25": HALVES_GONE,
    "absorb_pct 26": HALVES_KEPT,
    "over an unconfident row": dict(instance_mask=[0, 1, 2, 2, 1, 0, 0, 0], num_det=2,
                                    det_xy=_rows(AXY[0], BXY[0], fill=ZXY), det_cls=_rows(0.25, 1.0, fill=0.0),
                                    det_points=_rows(2, 2), det_src=_rows(1, 2), det_row=Z8, b_row=_rows(1, fill=-1),
                                    b_count=_rows(2), b_known=Z8, merge_count=[1, 1, 0, 0]),
    "every point of an unconfident row": dict(instance_mask=[0, 2, 2, 2, 0, 0, 0, 0], num_det=2, det_points=_rows(0, 3),
                                              det_src=_rows(1, 2), b_row=_rows(1, fill=-1), b_count=_rows(3),
                                              b_known=Z8, merge_count=[1, 1, 0, 0]),
    "score borders": dict(instance_mask=[1, 1, 4, 4, 5, 5, 0, 0], num_det=5,
                          det_xy=_rows(*AXY_ODD[:3], BXY[1], BXY[2], fill=ZXY),
                          det_cls=_rows(0.5, HALF_DOWN, NAN_PAYLOAD, -0.0, NAN_PAYLOAD, fill=0.0),
                          det_points=_rows(2, 0, 0, 2, 2), det_src=_rows(1, 1, 1, 2, 2), det_row=_rows(0, 1, 2, 1, 2),
                          b_row=_rows(-1, 3, 4, fill=-1), b_count=_rows(2, 2, 2), b_known=_rows(2, 0, 0),
                          merge_count=[3, 2, 1, 0]),
    "absorb_pct 0": dict(instance_mask=Z8, num_det=0, det_xy=[ZXY] * 8, det_cls=[0.0] * 8, det_points=Z8, det_src=Z8,
                         det_row=Z8, b_row=[-1] * 8, b_count=_rows(3, 2, 1), b_known=Z8, merge_count=[0, 0, 3, 0]),
    "absorb_pct 101": dict(instance_mask=[0, 1, 1, 1, 1, 1, 1, 0], num_det=2, det_xy=_rows(AXY[0], BXY[0], fill=ZXY),
                           det_cls=_rows(0.75, 1.0, fill=0.0), det_points=_rows(6, 0), det_src=_rows(1, 2), det_row=Z8,
                           b_row=_rows(1, fill=-1), b_count=_rows(3), b_known=_rows(3), merge_count=[1, 1, 0, 0]),
    "B ids": dict(instance_mask=[0, 0, 0, 1, 1, 2, 2, 0], num_det=2, det_points=_rows(2, 2), b_row=_rows(0, 1, fill=-1),
                  b_count=_rows(2, 2), merge_count=[0, 2, 0, 0]),
    "A ids": dict(instance_mask=[3, 3, 3, 1, 1, 2, 2, 0], num_det=3, det_xy=_rows(AXY[0], AXY[1], BXY[0], fill=ZXY),
                  det_cls=_rows(0.75, 0.75, 1.0, fill=0.0), det_points=_rows(2, 2, 3), det_src=_rows(1, 1, 2),
                  det_row=_rows(0, 1, 0), b_row=_rows(2, fill=-1), b_count=_rows(3), b_known=Z8,
                  merge_count=[2, 1, 0, 0]),
    "num_det beyond N": dict(instance_mask=[8, 0, 0, 0, 0, 0, 0, 0], num_det=8, det_xy=AXY,
                             det_cls=[0.25] * 7 + [0.75], det_points=[0] * 7 + [1], det_src=[1] * 8,
                             det_row=list(range(8)), b_row=[-1] * 8, b_count=[0] * 7 + [2], b_known=[0] * 7 + [1],
                             merge_count=[8, 0, 8, 0]),
    "num_det below 0": dict(instance_mask=Z8, num_det=0, det_xy=[ZXY] * 8, det_cls=[0.0] * 8, det_points=Z8, det_src=Z8,
                            det_row=Z8, b_row=[-1] * 8, b_count=Z8, b_known=Z8, merge_count=[0, 0, 0, 0]),
    "empty row between": dict(instance_mask=[1, 1, 0, 0, 2, 2, 0, 0], num_det=2, det_xy=_rows(BXY[0], BXY[2], fill=ZXY),
                              det_points=_rows(2, 2), det_src=_rows(2, 2), det_row=_rows(0, 2),
                              b_row=_rows(0, -1, 1, fill=-1), b_count=_rows(2, 0, 2), merge_count=[0, 2, 1, 0]),
    "ranks": dict(instance_mask=[2, 2, 1, 1, 3, 3, 0, 0], num_det=3, det_xy=_rows(AXY[0], BXY[0], BXY[2], fill=ZXY),
                  det_points=_rows(2, 2, 2), det_src=_rows(1, 2, 2), det_row=_rows(0, 0, 2),
                  b_row=_rows(1, -1, 2, fill=-1), b_count=_rows(2, 2, 2), b_known=_rows(0, 2, 0),
                  merge_count=[1, 2, 1, 0]),
    "nA N - 1": dict(instance_mask=[8, 8, 0, 0, 0, 0, 0, 0], num_det=8, det_xy=AXY[:7] + [BXY[0]],
                     det_cls=[0.75] * 7 + [1.0], det_points=[0] * 7 + [2], det_src=[1] * 7 + [2],
                     det_row=list(range(7)) + [0], b_row=_rows(7, -2, fill=-1), b_count=_rows(2, 2), b_known=Z8,
                     merge_count=[7, 1, 0, 1]),
    "nA N": dict(instance_mask=[0, 0, 0, 0, 5, 5, 0, 0], num_det=8, det_xy=AXY, det_cls=[0.25] * 8,
                 det_points=_rows(0, 0, 0, 0, 2), det_src=[1] * 8, det_row=list(range(8)), b_row=_rows(-2, -2, fill=-1),
                 b_count=_rows(2, 2), b_known=Z8, merge_count=[8, 0, 0, 2]),
    "N 1": dict(instance_mask=[1], num_det=1, det_xy=[BXY[0]], det_cls=[1.0], det_points=[1], det_src=[2], det_row=[0],
                b_row=[0], b_count=[1], b_known=[0], merge_count=[0, 1, 0, 0]),
    "N 1 with A": dict(instance_mask=[1], num_det=1, det_xy=[AXY[0]], det_cls=[0.75], det_points=[1], det_src=[1],
                       det_row=[0], b_row=[-1], b_count=[1], b_known=[1], merge_count=[1, 0, 1, 0]),
}
# the rule turned round in the restatement (its ``flip``) -> a scene whose outputs change
FLIPS = {"absorb >": "absorb_pct 25", "confident >": "score borders", "takes confident": "2 of 4 and 1 of 4",
         "empty kept": "empty row between", "capacity <=": "nA N - 1"}


@pytest.fixture(scope="module")
def rules():
    return {k: run_case(c) for k, c in rule_scenes().items()}


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_rule_scene_has_its_literal_values(rules, name):
    got = rules[name]
    assert tuple(got) == OUT_FIELDS
    for k, dt in zip(OUT_FIELDS, OUT_DTYPES):
        assert got[k].dtype == dt, k
    for k, want in EXPECTED[name].items():
        assert same_bits(got[k], np.asarray(want, got[k].dtype)), (name, k, got[k].tolist())
    assert sorted(EXPECTED) == sorted(rule_scenes())


def test_what_the_scenes_are_for(rules):
    # equality absorbs: 100 * 1 == 25 * 4; one per cent beyond it the row is kept
    assert rules["absorb_pct 25"]["merge_count"].tolist() == [1, 0, 2, 0]
    assert rules["absorb_pct 26"]["merge_count"].tolist() == [1, 1, 1, 0]
    # a kept row's known point keeps A's id
    o = rules["2 of 4 and 1 of 4"]
    assert o["instance_mask"][4] == 1 and o["b_known"][1] == 1 and o["det_points"][1] == 3 < o["b_count"][1]
    # an unconfident row's det_points falls, once to 0
    assert rules["over an unconfident row"]["det_points"][0] == 2
    assert rules["every point of an unconfident row"]["det_points"][0] == 0
    # a wholly known row that is appended all the same carries no point
    assert rules["absorb_pct 101"]["det_points"][1] == 0 and rules["absorb_pct 101"]["det_src"][1] == 2
    # the bits of A's rows and of the appended scores, NaN payloads and negative zeros included
    o = rules["score borders"]
    assert o["det_cls"].view(np.uint64)[2] == 0x7FF8000000000123 == o["det_cls"].view(np.uint64)[4]
    assert np.signbit(o["det_xy"][0, 0]) and np.signbit(o["det_cls"][3]) and o["det_cls"][3] == 0.0
    for name, o in rules.items():
        N, nd = len(o["instance_mask"]), int(o["num_det"])
        nA, appended, absorbed, dropped = o["merge_count"].tolist()
        nB = _clamp(rule_scenes()[name]["b"][1], N)
        assert nd == nA + appended <= N and appended + absorbed + dropped == nB, name
        for k in ("det_xy", "det_cls", "det_points", "det_src", "det_row"):
            assert not o[k][nd:].view(np.uint8 if o[k].dtype == np.uint8 else np.int64
                                      if o[k].dtype == np.float64 else np.int32).any(), (name, k)
        assert (o["b_row"][nB:] == -1).all() and not o["b_count"][nB:].any() and not o["b_known"][nB:].any(), name
        assert (o["det_src"][:nA] == 1).all() and (o["det_src"][nA:nd] == 2).all(), name
        assert o["det_points"].sum() == (o["instance_mask"] > 0).sum(), name
        assert sorted(o["b_row"][o["b_row"] >= 0].tolist()) == list(range(nA, nd)), name
        assert (o["b_row"] == -2).sum() == dropped, name


@pytest.mark.parametrize("flip", sorted(FLIPS))
def test_every_rule_is_held_by_a_scene(rules, flip):
    name = FLIPS[flip]
    flipped = run_case(rule_scenes()[name], flip=flip)
    changed = [k for k in OUT_FIELDS if not same_bits(flipped[k], rules[name][k])]
    assert changed, (flip, name)
    print("%s: changes %s of %r" % (flip, changed, name))


# ---------------------------------------------------------------- seeded patterns, for the device
PATTERN_N = (64, 65, 512, 513, 4096)


def _runs(rng, N, run, gap):
    """ids [N]: runs of equal ids 1, 2, ... in beam order, ``run()`` long with ``gap()`` zeros between them."""
    ids, i, k = np.zeros(N, np.int32), 0, 0
    while i < N:
        n = run()
        k += 1
        ids[i:i + n] = k
        i += n + gap()
    return ids, int(ids.max())


def _pattern(seed, N, fill=None):
    """B: runs of 1-5 points with gaps of 0-2 (more than N / 8 rows), one forced over the points 62-65 and one over
    510-513, a few ids nobody's, some rows without a point.  A: runs of 4-24 points, half of them confident, so kept and
    absorbed B rows alternate all along the scan.  ``fill``: a_num_det is raised -- the added rows are not confident, so
    who is kept does not change -- until nA + kept is N (``"full"``) or N + 1 (``"over"``)."""
    rng = np.random.default_rng(seed)
    b_inst, nB = _runs(rng, N, lambda: int(rng.integers(1, 6)), lambda: int(rng.integers(0, 3)))
    free = np.ones(N, bool)
    for lo in (62, 510):
        if lo + 2 < N:
            b_inst[lo:lo + 4] = max(int(b_inst[:lo + 1].max()), 1)     # the run open at lo, or the one before it
            free[lo:lo + 4] = False
    spoil = rng.choice(np.flatnonzero(free), max(N // 16, 1), replace=False)
    b_inst[spoil] = rng.choice([0, -1, nB + 1, 2 ** 31 - 1], len(spoil))
    a_inst, nA = _runs(rng, N, lambda: int(rng.integers(4, 25)), lambda: int(rng.integers(0, 12)))
    a_inst[rng.choice(N, max(N // 32, 1), replace=False)] = nA + 1
    a_cls = np.zeros(N)
    a_cls[:nA] = rng.choice([0.75, 0.25, 0.5, HALF_DOWN, NAN], nA, p=[0.4, 0.3, 0.1, 0.1, 0.1])
    a_xy, b_xy = rng.standard_normal((N, 2)), rng.standard_normal((N, 2))
    a_xy[rng.choice(N, 3)] = [-0.0, NAN_PAYLOAD]
    b_cls = np.where(np.arange(N) < nB, 1.0, 0.0)
    case = dict(b=(b_inst, np.int32(nB), b_xy, b_cls), a=(a_inst, np.int32(nA), a_xy, a_cls), kw=dict(DEFAULTS))
    if fill:
        kept = int((run_case(case)["b_row"] != -1).sum())
        n_a = N - kept + (fill == "over")
        assert n_a >= nA, (N, kept, nA)
        a_cls[nA:n_a] = 0.25                                   # row nA gets the points whose id was nobody's
        case["a"] = (a_inst, np.int32(n_a), a_xy, a_cls)
    return case


_PATTERNS = {}
# name -> (N, fill); REACHES: what each must reach, asserted below
PATTERNS = {"N 64": (64, None), "N 65": (65, None), "N 65 full": (65, "full"), "N 65 over": (65, "over"),
            "N 512": (512, None), "N 512 over": (512, "over"), "N 513": (513, None), "N 513 full": (513, "full"),
            "N 4096": (4096, None), "N 4096 full": (4096, "full"), "N 4096 over": (4096, "over")}
REACHES = {
    "N 64": ("interleaved",), "N 65": ("interleaved", "straddles 63/64"), "N 65 full": ("rows == N", "straddles 63/64"),
    "N 65 over": ("one dropped", "straddles 63/64"),
    "N 512": ("interleaved", "slots above 0", "both in every slot", "straddles 63/64"),
    "N 512 over": ("one dropped", "slots above 0"),
    "N 513": ("interleaved", "straddles 63/64", "straddles 511/512"), "N 513 full": ("rows == N", "straddles 511/512"),
    "N 4096": ("interleaved", "slots above 0", "both in every slot", "straddles 63/64", "straddles 511/512"),
    "N 4096 full": ("rows == N", "slots above 0"), "N 4096 over": ("one dropped", "slots above 0"),
}


def pattern_cases():
    """-> {name: case}: what tests/test_merge_detections_gpu.py runs besides the rule scenes.  Built once."""
    if not _PATTERNS:
        for n, (name, (N, fill)) in enumerate(PATTERNS.items()):
            _PATTERNS[name] = _pattern(180 + PATTERN_N.index(N), N, fill)
    return _PATTERNS


def test_pattern_cases_reach_what_the_table_says():
    cases = pattern_cases()
    assert sorted(REACHES) == sorted(cases) and {N for N, _ in PATTERNS.values()} == set(PATTERN_N)
    for name, case in cases.items():
        o = run_case(case)
        N = len(o["instance_mask"])
        threads = 64 if N <= 512 else 512
        nB = _clamp(case["b"][1], N)
        nA, appended, absorbed, dropped = o["merge_count"].tolist()
        kept = o["b_row"][:nB] != -1
        print("%s: nA %d, nB %d, appended %d, absorbed %d, dropped %d, points that changed rows %d"
              % (name, nA, nB, appended, absorbed, dropped,
                 int((o["instance_mask"] != np.where((case["a"][0] >= 1) & (case["a"][0] <= nA), case["a"][0], 0)).sum())))
        members = lambda a, b: case["b"][0][a] == case["b"][0][b] and 1 <= case["b"][0][a] <= nB
        reached = {
            "interleaved": bool((kept[:-1] != kept[1:]).sum() >= 2) and o["b_known"].any() and appended > 0,
            "slots above 0": nB > threads,
            "both in every slot": all(kept[c:c + threads].any() and not kept[c:c + threads].all()
                                      for c in range(0, nB - threads // 2, threads)),
            "straddles 63/64": N > 64 and members(63, 64),
            "straddles 511/512": N > 512 and members(511, 512),
            "rows == N": nA + int(kept.sum()) == N and dropped == 0 and int(o["num_det"]) == N,
            "one dropped": nA + int(kept.sum()) == N + 1 and dropped == 1 and int(o["num_det"]) == N,
        }
        for what in REACHES[name]:
            assert reached[what], (name, what)
        if name == "N 4096":
            assert nB > 512
    # the five flips change the patterns too
    for flip in FLIPS:
        assert any(not same_bits(run_case(c, flip=flip)[k], run_case(c)[k]) for c in cases.values() for k in OUT_FIELDS)


# ---------------------------------------------------------------- what the merge is good for
QUALITY_SEEDS = (1, 2, 3, 4, 5, 6)
QUALITY_STEPS = (0.25, 0.06)
LOWERED = 0.1                                                  # a net that sees them but is not confident


def lowered_scene(seed, T, max_step):
    """``people_scene`` with the NMS score of every odd-numbered person (p = 1, 3, 5) lowered to 0.1 in every scan.
    -> (the scene, the numbers of the lowered people)."""
    scene = people_scene(seed, T, max_step)
    low = list(range(1, scene["rows"].shape[1], 2))
    for t, s in enumerate(scene["scans"]):
        s["det_cls"] = s["det_cls"].copy()
        s["det_cls"][scene["rows"][t, low]] = LOWERED
    return scene, low


def merged_chain(scene, gate, absorb_pct=50):
    """cast -> segments (with the scene's NMS record) -> merge -> grid map over a scene, 256 x 256 cells of 0.1 m and
    defaults; ``gate``: "nms" or "merged", the record that gates the grid map.  -> per scan (segments, merged)."""
    H = W = 256
    res = 0.1
    origin = scene["poses"][0, :2] - 0.5 * res * np.array([W, H])
    grid = np.zeros((H, W), np.int16)
    steps = []
    for s in scene["scans"]:
        nms = (s["inst"], s["num_det"], s["det_cls"])
        cast = grid_cast_oracle(s["ranges"], scene["tab"], s["rot"], s["trans"], grid, origin, res)
        seg = novel_segments_oracle(s["ranges"], scene["tab"], cast["point_class"], *nms)
        o = merge_detections_oracle(seg["instance_mask"], seg["num_det"], seg["det_xy"], seg["det_cls"], s["inst"],
                                    s["num_det"], s["det_xy"], s["det_cls"], absorb_pct=absorb_pct)
        by = nms if gate == "nms" else (o["instance_mask"], o["num_det"], o["det_cls"])
        grid_map_oracle(s["ranges"], scene["tab"], s["rot"], s["trans"], grid, origin, res, *by)
        steps.append((seg, o))
    return steps


def _quality(scene, low, gate):
    """-> (person-scans of the lowered people found by an appended row over scans 12-23, person-scans there are, wall
    points in appended rows and points of confident people in appended rows over all scans)."""
    found = there = wall = confident = 0
    for t, (s, (_, o)) in enumerate(zip(scene["scans"], merged_chain(scene, gate))):
        appended = o["instance_mask"] > o["merge_count"][0]
        wall += int((appended & (s["inst"] == 0)).sum())
        for p in range(scene["rows"].shape[1]):
            mine = s["inst"] == scene["rows"][t, p] + 1
            if p not in low:
                confident += int((appended & mine).sum())
            elif t >= 12:
                found, there = found + bool((appended & mine).any()), there + 1
    return found, there, wall, confident


def test_quality_on_rooms_with_lowered_people():
    """Conditions: no wall point (inst == 0) and no point of a person whose score was left confident lies in an appended
    row, on any scan of the 24 runs; per seed the map gated by the merged record finds at least as many person-scans of
    the lowered people as the map gated by the NMS record alone; over the six seeds at max_step 0.25 it finds some.  The
    counts are printed, not asserted.  Measured with this restatement (recorded in DESIGN.md 8, N18), person-scans of
    the lowered people found by an appended row over scans 12-23 per seed 1-6: max_step 0.25 (of 12, 24, 24, 12, 12, 12):
    gated by the NMS record 2, 0, 9, 2, 0, 4; by the merged record 4, 0, 11, 10, 0, 12.  max_step 0.06 (of 12 each): 7, 0,
    8, 0, 0, 0; 12, 0, 12, 0, 0, 0.  Every cell is the figure of the prototype the stage was specified from."""
    for step in QUALITY_STEPS:
        table = {"nms": [], "merged": []}
        for seed in QUALITY_SEEDS:
            scene, low = lowered_scene(seed, 24, step)
            for gate in table:
                found, there, wall, confident = _quality(scene, low, gate)
                table[gate].append((found, there))
                assert wall == 0 and confident == 0, (step, seed, gate, wall, confident)
            assert table["merged"][-1][0] >= table["nms"][-1][0], (step, seed)
        for gate in table:
            print("max_step %.2f, map gated by the %-6s record: lowered person-scans found per seed %s of %s"
                  % (step, gate, [f for f, _ in table[gate]], [n for _, n in table[gate]]))
        if step == 0.25:
            assert sum(f for f, _ in table["merged"]) > 0


def test_confident_detections_are_tracked_as_without_the_merge():
    """By construction: a confident detection keeps its row, its centre and all its points.  On the scenes as they are
    (nobody lowered) the merged record therefore gives ``person_motion_oracle`` and ``track_step`` what the NMS record
    gives them: every per-row output on the rows < nA, and with no appended row every field of the track state."""
    for seed in (1, 2, 3):
        scene = people_scene(seed, 12, 0.25)
        N, M = len(scene["scans"][0]["ranges"]), 16
        pm = {k: motion_state(N) for k in ("nms", "merged")}
        tr = {k: new_track_state(M, N) for k in ("nms", "merged")}
        appended = 0
        for t, (s, (_, o)) in enumerate(zip(scene["scans"], merged_chain(scene, "merged"))):
            nA = int(o["merge_count"][0])
            appended += int(o["merge_count"][1])
            assert nA == int(s["num_det"]) and same_bits(o["det_xy"][:nA], s["det_xy"][:nA]) and \
                same_bits(o["det_cls"][:nA], s["det_cls"][:nA])
            own = (s["inst"] >= 1) & (s["inst"] <= nA)
            assert np.array_equal(o["instance_mask"][own], s["inst"][own])     # all its points
            recs = {"nms": (s["inst"], s["num_det"], s["det_xy"], s["det_cls"]),
                    "merged": (o["instance_mask"], o["num_det"], o["det_xy"], o["det_cls"])}
            outs = {k: person_motion_oracle(s["ranges"], scene["tab"], *recs[k], s["rot"], s["trans"], pm[k]) for k in recs}
            for k, v in outs["nms"].items():
                assert same_bits_nan(np.asarray(v)[:nA], np.asarray(outs["merged"][k])[:nA]), (seed, t, k)
            for k in recs:
                track_step(tr[k], outs[k]["det_xy_world"], outs[k]["det_flow"], outs[k]["det_valid"], recs[k][1],
                           recs[k][0])
            assert np.array_equal(tr["nms"]["det_track"][:nA], tr["merged"]["det_track"][:nA]), (seed, t)
            if appended == 0:
                for k in TRACK_INT + TRACK_FLOAT:
                    assert same_bits_nan(tr["nms"][k], tr["merged"][k]), (seed, t, k)
        print("seed %d: %d appended rows over 12 scans, %d tracks" % (seed, appended, int(tr["merged"]["next_id"]) - 1))
        assert int(tr["merged"]["next_id"]) > 1


# ---------------------------------------------------------------- surface
RECORD = (("instance_mask", "int32", (2, 5)), ("num_det", "int32", (2,)), ("det_xy", "float64", (2, 5, 2)),
          ("det_cls", "float64", (2, 5)), ("det_points", "int32", (2, 5)), ("det_src", "uint8", (2, 5)),
          ("det_row", "int32", (2, 5)), ("b_row", "int32", (2, 5)), ("b_count", "int32", (2, 5)),
          ("b_known", "int32", (2, 5)), ("merge_count", "int32", (2, 4)))
DETECTOR_DEFAULTS = dict(absorb_pct=50, gate_map=True)


def test_record_and_settings_match_literal_tables():
    import torch
    from planar_optical_flow_amd import ops, streaming
    rec = ops.merge_detections_buffers(2, 5, device="cpu")
    assert type(rec) is ops.MergedDetections and type(rec).__name__ == "MergedDetections"
    assert ops.MergedDetections.persistent == ()
    assert rec._fields == tuple(f for f, _, _ in RECORD) == OUT_FIELDS
    for (f, dtype, shape), t in zip(RECORD, rec):
        assert (t.dtype, tuple(t.shape), t.device.type) == (getattr(torch, dtype), shape, "cpu") and not t.any(), f
    got = ops.stage_settings(ops.merge_detections)
    assert got == DEFAULTS and list(got) == list(DEFAULTS)
    assert {k: type(v) for k, v in got.items()} == {k: type(v) for k, v in DEFAULTS.items()}
    assert streaming.stage_defaults("merge_detections") == DETECTOR_DEFAULTS
    assert streaming.stage_defaults("merge_detections", 0.7, "keyframe") == DETECTOR_DEFAULTS
    assert streaming.stage_settings("merge_detections", dict(absorb_pct=30, gate_map=False)) == \
        dict(absorb_pct=30, gate_map=False)
    for unknown in ("cls_thresh", "res", "absorb"):
        with pytest.raises(ValueError, match="unknown merge_detections settings"):
            streaming.stage_settings("merge_detections", {unknown: 0.5})
    # the stage beside it keeps its table
    assert streaming.stage_defaults("novel_segments") == dict(jump=0.3, max_skip=2, min_points=3, max_width=1.0,
                                                              gate_map=False)


def test_header_binding_and_wrappers():
    import torch
    from planar_optical_flow_amd import _lib, ops
    from planar_optical_flow_amd.src.utils import utils
    from planar_optical_flow_amd.streaming import StreamingDetector
    text = open(os.path.join(REPO, "include", "pof_abi.h")).read()
    m = re.search(r"\bint\s+pof_merge_detections\s*\(([^)]*)\)\s*;", text)
    assert m, "include/pof_abi.h does not declare pof_merge_detections"
    params = [p.strip() for p in m.group(1).split(",")]
    restype, argtypes = _lib.SIGNATURES["pof_merge_detections"]
    assert restype is _lib._i and len(argtypes) == len(params) == 24
    for p, t in zip(params, argtypes):
        want = _lib._p if "*" in p or p.startswith("pof_stream_t") else _lib._d if p.startswith("double") else _lib._i
        assert t is want, p
    # the outputs of the prototype are the record's fields, in its order
    assert [p.split("*")[-1].strip() for p in params[12:23]] == list(OUT_FIELDS)
    assert [p.split("*")[-1].strip() for p in params[:8]] == \
        [s + f for s in ("b_", "a_") for f in ("instance_mask", "num_det", "det_xy", "det_cls")]
    assert "N18" in text and "absorb_pct" in text
    p = inspect.signature(ops.merge_detections).parameters
    assert list(p) == ["b_instance_mask", "b_num_det", "b_det_xy", "b_det_cls", "instance_mask", "num_det", "det_xy",
                       "det_cls", "cls_thresh", "absorb_pct", "out"]
    assert {k: p[k].default for k in DEFAULTS} == DEFAULTS and p["out"].default is None
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[4:])
    assert [p[k].default for k in ("instance_mask", "num_det", "det_xy", "det_cls")] == [None] * 4
    assert list(inspect.signature(ops.merge_detections_buffers).parameters) == ["B", "N", "device"]
    # the first four fields are person_motion's arguments behind the table, in its order
    assert list(inspect.signature(ops.person_motion).parameters)[2:6] == list(OUT_FIELDS[:4])
    assert list(inspect.signature(utils.OccupancyGrid.merged_detections).parameters)[1:] == \
        ["scan", "odom", "pred_cls", "pred_reg", "settings"]
    assert inspect.signature(StreamingDetector.__init__).parameters["merge_detections"].default is None
    assert callable(StreamingDetector.merged_detections)
    # no CPU path
    cpu = (torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
           torch.zeros(1, 4, 2, dtype=torch.float64), torch.zeros(1, 4, dtype=torch.float64))
    with pytest.raises(TypeError):
        ops.merge_detections(*cpu)
    with pytest.raises(TypeError):
        ops.merge_detections(None, None, None, None)


def test_entry_point_refuses_null_and_bad_arguments():
    import ctypes
    from planar_optical_flow_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH) and not os.path.exists(build.HIPCC):
        pytest.skip("the library is not built and there is no hipcc to build it")
    build.build(verbose=False)
    lib = _lib.load()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "pof_merge_detections")
    _, argtypes = _lib.SIGNATURES["pof_merge_detections"]
    assert lib.pof_merge_detections(*[None if t is _lib._p else 0 for t in argtypes]) == _lib.POF_E_BADARG
    assert lib.pof_merge_detections(*[None if t is _lib._p else 1 for t in argtypes]) == _lib.POF_E_BADARG
    # with pointers (never followed: every call below is refused, or B is 0): which refusal, and their order
    word = ctypes.cast((ctypes.c_double * 4)(), ctypes.c_void_p)
    good = dict(b=(word,) * 4, a=(word,) * 4, cls_thresh=0.5, absorb_pct=50, B=0, N=8, out=(word,) * 11)

    def call(**kw):
        v = dict(good, **kw)
        return lib.pof_merge_detections(*v["b"], *v["a"], v["cls_thresh"], v["absorb_pct"], v["B"], v["N"], *v["out"],
                                        None)

    assert call() == _lib.POF_OK and call(a=(None,) * 4) == _lib.POF_OK                # B = 0 with valid pointers
    assert call(absorb_pct=0, N=4096) == _lib.POF_OK and call(absorb_pct=101, N=1) == _lib.POF_OK
    assert call(cls_thresh=NAN) == _lib.POF_OK                  # any score threshold is legal: nobody is confident
    part = [tuple(None if i == j else word for i in range(4)) for j in range(4)] + \
        [tuple(word if i == j else None for i in range(4)) for j in range(4)]
    for bad in [dict(a=a) for a in part] + [dict(b=b) for b in part[:4]] + \
            [dict(out=tuple(None if i == j else word for i in range(11))) for j in range(11)] + \
            [dict(absorb_pct=-1), dict(absorb_pct=102), dict(B=-1), dict(N=0), dict(absorb_pct=102, N=4097)]:
        assert call(**bad) == _lib.POF_E_BADARG, bad            # BADARG is checked first
    assert call(N=4097) == _lib.POF_E_SHAPE
