"""The association paths of the flat scan kernel (scan_flat_kernel), each on inputs built to take it.

The kernel decides most points with a float32 screen: a packed minimum over the sample's detections, then ONE packed
pass that names the candidate of both points of a lane, then -- for points in an error band, under two discs, beyond
100 m or in a sample with a far detection -- the exact float64 loop; winners beyond inline slot 7 come from the CSR
table, and the regression targets of a lane's two points are computed in one block.  Every case below is a few
samples of 128, 130 or 450 points (one wave = 128 points of the flat [B * N] axis: exactly one sample, a wave that
wraps into the next sample at lane 1, the production length), is compared with oracle/ref_numpy.py only (closest,
target_cls, dyn_mask, exclude_mask exactly, target_reg at atol 1e-6), and first asserts FROM THE ORACLE ALONE that
the situation it is meant to hit occurs in its inputs.  Each case runs as float32 outputs through
ops.scan_preprocess_multi (two slots of different size and detection count, so the slot of a wave is found by the
search; the float32 beam table) and as float64 outputs through ops.scan_preprocess.

A rim is a detection on a beam's bearing at range r_i +- radius.  Its float64 distance to the beam's point is the
radius up to the rounding of the two products (about 1e-15 m), far inside the float32 screen's band (about 1e-3 m^2 of
squared distance), so the exact loop decides and the oracle's answer is the expected one.  Next to each exact rim sit
two more whose range is moved by radius * 1e-9 to either side: still inside the band, but decided the same way by
any correctly rounded arithmetic.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import ref_numpy as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
RA = (0.6, 0.4, 0.35)       # association radius per class (wc, wa, wp): the defaults of ops and of the oracle
RD = (2.5, 2.0, 2.0)        # dynamic-mask radius per class
FULL = ("flow", "closest", "target_cls", "target_reg", "dyn_mask", "exclude_mask")
HEADLINE = ("flow", "target_cls", "target_reg", "exclude_mask")
SIZES = (128, 130, 450)


@pytest.fixture(scope="module")
def ops():
    from planar_optical_flow_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _ops


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def base_scan(N):
    return (12.0 + 0.01 * np.sin(0.37 * np.arange(N))).astype(np.float32)


def on_beam(scan, phi, i, dr=0.0, cls=2, dphi=0.0):
    """A detection (r, phi, class) on the bearing of beam i, dr behind its point."""
    return (float(scan[i]) + dr, float(phi[i]) + dphi, cls)


def sample(scan, dets):
    dets = sorted(dets, key=lambda d: d[2])     # CSR order = the oracle's: wc, wa, wp
    return {"scan": scan, "dets": dets}


def distances(s, phi):
    """[N, D] float64 distances point -> detection centre, with the oracle's operations."""
    px, py = R.polar_to_xy(s["scan"], phi)
    d = np.empty((len(phi), len(s["dets"])))
    for k, (dr, dphi, _) in enumerate(s["dets"]):
        cx, cy = R.polar_to_xy(dr, dphi)
        d[:, k] = np.sqrt((px - cx) ** 2 + (py - cy) ** 2)
    return d


def oracle(s, phi):
    scan = s["scan"]
    by = [[(r, p) for (r, p, c) in s["dets"] if c == k] for k in range(3)]
    with np.errstate(all="ignore"):
        closest = R.closest_detection(scan, phi, by[0] + by[1] + by[2],
                                      [RA[0]] * len(by[0]) + [RA[1]] * len(by[1]) + [RA[2]] * len(by[2]))
        cls, reg = R.regression_target(scan, phi, by[0], by[1], by[2])
        xy = np.array(R.polar_to_xy(scan, phi)).T
        dyn = R.dynamic_mask(xy, by[0], by[1], by[2])
        exc = dyn * R.valid_point_mask(scan)
        dist = distances(s, phi)
    return {"closest": np.asarray(closest, dtype=np.int64), "target_cls": cls, "target_reg": reg, "dyn_mask": dyn,
            "exclude_mask": exc, "dist": dist}


# ---------------------------------------------------------------- the cases: (samples, check(samples, expected))
def _rims(N, phi, radii):
    """One sample per class; six detections each: r_i + rad and r_i - rad, exact and moved by rad * 1e-9 inwards and
    outwards.  rim = (beam, detection, radius, -1 inside / 0 exact / +1 outside)."""
    samples, rims = [], []
    for c in range(3):
        scan = base_scan(N)
        dets, mine = [], []
        k = 0
        for sign in (1.0, -1.0):
            for side in (0, -1, 1):
                i = (k + 1) * N // 7
                dets.append(on_beam(scan, phi, i, sign * radii[c] * (1.0 + side * 1e-9), c))
                mine.append((i, k, radii[c], side))
                k += 1
        samples.append(sample(scan, dets))
        rims.append(mine)
    return samples, rims


def _check_rims(exp, rims, decided):
    for e, mine in zip(exp, rims):
        for (i, k, rad, side) in mine:
            gap = e["dist"][i, k] - rad
            if side == 0:
                assert abs(gap) <= 1e-9, (i, k, gap)          # the tie: rounding noise of the float64 products
            else:
                assert 1e-11 < side * gap < 1e-8, (i, k, gap)  # beside the tie, inside the float32 band
                assert decided(e, i, k) == (side < 0), (i, k)
            # nothing else lies near a rim at this point: the decision is this detection's
            others = np.delete(np.abs(e["dist"][i] - rad), k)
            assert others.min() > 1e-3, (i, k)


def case_rims_assoc(N, phi):
    samples, rims = _rims(N, phi, RA)

    def check(exp):
        _check_rims(exp, rims, lambda e, i, k: e["closest"][i] == k + 1)
    return samples, check


def case_rims_dyn(N, phi):
    samples, rims = _rims(N, phi, RD)

    def check(exp):
        _check_rims(exp, rims, lambda e, i, k: e["dyn_mask"][i] == 0.0)
        for e in exp:
            assert (e["closest"] == 0).all()                  # 2 m away: the dynamic mask alone is at stake
    return samples, check


def case_two_discs(N, phi):
    ia, ib = 2 * (N // 6), 2 * (N // 3) + 1                   # a point 0 and a point 1 of their lanes
    dl = 0.1 / 12.0
    s0 = base_scan(N)
    d0 = [on_beam(s0, phi, ia, 0.05), on_beam(s0, phi, ia, 0.25), on_beam(s0, phi, ib, 0.25), on_beam(s0, phi, ib, 0.05)]
    s1 = base_scan(N)
    d1 = [on_beam(s1, phi, ia, dphi=dl), on_beam(s1, phi, ia, dphi=-dl),
          on_beam(s1, phi, ib, dphi=-dl), on_beam(s1, phi, ib, dphi=dl)]
    s2 = base_scan(N)
    d2 = [on_beam(s2, phi, ia, RA[0], 0), on_beam(s2, phi, ia, -0.2, 2),
          on_beam(s2, phi, ib, RA[2], 2), on_beam(s2, phi, ib, 0.1, 1)]
    samples = [sample(s0, d0), sample(s1, d1), sample(s2, d2)]

    def check(exp):
        rad = [np.array([RA[c] for (_, _, c) in s["dets"]]) for s in samples]
        for i in (ia, ib):
            # two detections 0.2 m apart, the point inside both discs
            inside = np.flatnonzero(exp[0]["dist"][i] < rad[0] - 0.05)
            assert len(inside) == 2 and exp[0]["closest"][i] == inside[np.argmin(exp[0]["dist"][i][inside])] + 1
            # mirrored about the beam: equal distances, the first minimum wins
            inside = np.flatnonzero(exp[1]["dist"][i] < rad[1] - 0.05)
            assert len(inside) == 2 and abs(np.diff(exp[1]["dist"][i][inside])[0]) <= 1e-12
            assert exp[1]["closest"][i] in (inside + 1)
            # one of the two on its rim (in the band), the other well inside
            gap = exp[2]["dist"][i] - rad[2]
            assert (np.abs(gap) <= 1e-9).sum() == 1 and (gap < -0.05).sum() == 1
            assert exp[2]["closest"][i] == np.argmin(gap) + 1
    return samples, check


def case_slots(N, phi):
    p = [(k + 1) * N // 14 for k in range(12)]
    s0 = base_scan(N)
    d0 = [on_beam(s0, phi, p[k]) for k in range(12)]
    s1 = base_scan(N)
    e = p[7] & ~1
    s1[e + 1] = 14.0
    beams = p[:7] + [e, e + 1] + p[9:]
    d1 = [on_beam(s1, phi, b, cls=(0 if k < 3 else 1 if k < 6 else 2)) for k, b in enumerate(beams)]
    s2 = base_scan(N)
    d2 = [on_beam(s2, phi, p[k]) for k in range(8)]
    samples = [sample(s0, d0), sample(s1, d1), sample(s2, d2)]

    def check(exp):
        # winner in inline slot 7, in the first CSR slot, in the last of 12
        assert [exp[0]["closest"][p[k]] for k in (7, 8, 11)] == [8, 9, 12]
        # one lane, two winners: inline slot 7 for its point 0, CSR slot 8 for its point 1
        assert e % 2 == 0 and exp[1]["closest"][e] == 8 and exp[1]["closest"][e + 1] == 9
        assert exp[1]["target_cls"][e] == 3 and len(set(exp[1]["target_cls"])) == 4
        assert len(samples[2]["dets"]) == 8 and exp[2]["closest"][p[7]] == 8
    return samples, check


def case_one_point(N, phi):
    s0 = base_scan(N)
    s0[1::2] = 15.0
    a, b = 2 * (N // 8), 2 * (3 * N // 8) + 1
    samples = [sample(s0, [on_beam(s0, phi, a), on_beam(s0, phi, b)]), sample(base_scan(N), [])]

    def check(exp):
        c = exp[0]["closest"]
        assert c[a] == 1 and c[a + 1] == 0          # a lane where only point 0 has a winner
        assert c[b] == 2 and c[b - 1] == 0          # a lane where only point 1 has
        assert (c[0::2] <= 1).all() and (c[1::2] != 1).all()
    return samples, check


def case_straddle(N, phi):
    counts = (0, 8, 0, 3, 12)
    samples = []
    for n in counts:
        scan = base_scan(N)
        beams = np.round(np.linspace(1, N - 2, n)).astype(int) if n else []
        samples.append(sample(scan, [on_beam(scan, phi, int(i)) for i in beams]))

    def check(exp):
        for b in range(len(counts) - 1):
            # the wave that holds the end of sample b and the start of sample b + 1 has associated points of
            # every one of the two that has detections: counts (0, 8), (8, 0), (0, 3), (3, 12)
            w = ((b + 1) * N) // 128
            assert ((b + 1) * N) % 128 != 0
            tail = np.arange(128 * w, (b + 1) * N) - b * N
            head = np.arange((b + 1) * N, min(128 * (w + 1), (b + 2) * N)) - (b + 1) * N
            assert len(tail) and len(head)
            assert (exp[b]["closest"][tail] > 0).any() == (counts[b] > 0)
            assert (exp[b + 1]["closest"][head] > 0).any() == (counts[b + 1] > 0)
    return samples, check


def case_exact(N, phi):
    p = [(k + 1) * N // 5 for k in range(3)]
    s0 = base_scan(N)
    d0 = [on_beam(s0, phi, i) for i in p] + [(150.0, float(phi[N // 2]), 2)]
    i0 = 2 * (N // 4)
    s1 = base_scan(N)
    s1[i0] = 120.0
    d1 = [on_beam(s1, phi, i0 + 2)]
    s2 = base_scan(N)
    s2[i0 + 1] = np.inf
    d2 = [on_beam(s2, phi, i0 + 2)]
    samples = [sample(s0, d0), sample(s1, d1), sample(s2, d2)]

    def check(exp):
        # a detection beyond 100 m: the whole sample takes the exact loop, and still finds its three people
        assert max(r for (r, _, _) in samples[0]["dets"]) > 100.0
        assert [exp[0]["closest"][i] for i in p] == [1, 2, 3] and (exp[0]["closest"] != 4).all()
        # a range of 120 m / an infinite range, its lane partner and its neighbours associated: the same wave
        for k, bad in ((1, i0), (2, i0 + 1)):
            assert not samples[k]["scan"][bad] < 100.0
            c = exp[k]["closest"]
            assert c[bad] == 0 and c[bad ^ 1] == 1 and c[i0 + 2] == 1 and c[i0 + 3] == 1
            assert (k * N + i0) // 128 == (k * N + i0 + 3) // 128
            assert exp[k]["exclude_mask"][bad] == 0.0
    return samples, check


CASES = {"rims_assoc": case_rims_assoc, "rims_dyn": case_rims_dyn, "two_discs": case_two_discs, "slots": case_slots,
         "one_point": case_one_point, "straddle": case_straddle, "exact": case_exact}
PARAMS = [(name, N) for name in CASES for N in SIZES if not (name == "straddle" and N % 128 == 0)]


@functools.lru_cache(maxsize=None)
def built(name, N):
    """(samples, expected per sample): the oracle runs once per case and size, after the case's own check."""
    phi = R.laser_phi(num_pts=N)
    samples, check = CASES[name](N, phi)
    assert 2 <= len(samples) <= 5
    exp = [oracle(s, phi) for s in samples]
    check(exp)
    return samples, exp


# ---------------------------------------------------------------- the two entry points
def device_batch(ops, samples, N, out_dtype, want):
    B = len(samples)
    offs = np.concatenate([[0], np.cumsum([len(s["dets"]) for s in samples])]).astype(np.int32)
    rphi = np.array([[r, p] for s in samples for (r, p, _) in s["dets"]], dtype=np.float64).reshape(-1, 2)
    cls = np.array([c for s in samples for (_, _, c) in s["dets"]], dtype=np.uint8)
    det = ops.DetCSR.from_numpy(offs, rphi, cls, DEV)
    odom0 = np.array([[0.1 * b, -0.05 * b, 0.02 * b] for b in range(B)])
    odom1 = odom0 + np.array([0.03, 0.01, 0.015])
    shapes = {"flow": ((B, N, 2), out_dtype), "closest": ((B, N), torch.int64), "target_cls": ((B, N), torch.int64),
              "target_reg": ((B, N, 2), torch.float32), "dyn_mask": ((B, N), torch.float32),
              "exclude_mask": ((B, N), torch.float32)}
    out = {k: torch.full(shapes[k][0], 7, dtype=shapes[k][1], device=DEV) for k in want}
    ws = torch.empty(ops.scan_preprocess_workspace_bytes(B, det.rphi.shape[0]), dtype=torch.uint8, device=DEV)
    return {"scans": T(np.stack([s["scan"] for s in samples])), "odom0": T(odom0), "odom1": T(odom1), "dets": det,
            "workspace": ws, "out": out}


def compare(out, exp, want, tag):
    got = {k: out[k].cpu().numpy() for k in want if k != "flow"}
    for b, e in enumerate(exp):
        for k in ("closest", "target_cls", "dyn_mask", "exclude_mask"):
            if k in got:
                bad = np.flatnonzero(got[k][b] != e[k])
                assert len(bad) == 0, (tag, k, b, bad[:8], got[k][b][bad[:8]], e[k][bad[:8]])
        np.testing.assert_allclose(got["target_reg"][b], e["target_reg"], rtol=0, atol=1e-6, err_msg=str((tag, b)))


def run_multi_f32(ops, samples, exp, N, want, flow_kind):
    """Two slots in one launch: the batch, and the batch without its last sample."""
    tab = ops.phi_table(num_pts=N)
    groups = [(samples, exp), (samples[:-1], exp[:-1])]
    slots = [device_batch(ops, s, N, torch.float32, want) for s, _ in groups]
    ops.scan_preprocess_multi([], tab, next_batches=slots, want=want, flow_kind=flow_kind)
    ops.scan_preprocess_multi(slots, tab, want=want, flow_kind=flow_kind)
    for k, (slot, (_, e)) in enumerate(zip(slots, groups)):
        compare(slot["out"], e, want, ("multi f32", sorted(want), k))


@pytest.mark.parametrize("name,N", PARAMS)
def test_assoc_paths_f32_multi(ops, name, N):
    samples, exp = built(name, N)
    run_multi_f32(ops, samples, exp, N, FULL, ops.FLOW_DISPLACEMENT)         # the run-time-flag instantiation
    run_multi_f32(ops, samples, exp, N, HEADLINE, ops.FLOW_DISPLACEMENT)     # the headline instantiation


@pytest.mark.parametrize("name,N", PARAMS)
def test_assoc_paths_f64_single(ops, name, N):
    samples, exp = built(name, N)
    d = device_batch(ops, samples, N, torch.float64, FULL)
    out = ops.scan_preprocess(d["scans"], ops.phi_table(num_pts=N), d["odom0"], d["odom1"], d["dets"],
                              out_dtype=torch.float64, want=FULL)
    compare(out, exp, FULL, "single f64")


@pytest.mark.parametrize("N", SIZES)
def test_assoc_paths_flow_target_f32(ops, N):
    """One sample of every case as flow_kind 1 with float32 outputs: that flow stays float64 arithmetic, the
    association is the shared code."""
    picks = (("rims_assoc", 2), ("two_discs", 2), ("slots", 1), ("one_point", 0), ("rims_dyn", 0), ("exact", 2))
    if N % 128:
        picks = picks + (("straddle", 4),)
    samples = [built(name, N)[0][k] for name, k in picks]
    exp = [built(name, N)[1][k] for name, k in picks]
    for lo, hi in ((0, 4), (4, len(samples))):
        run_multi_f32(ops, samples[lo:hi], exp[lo:hi], N, FULL, ops.FLOW_TARGET)
