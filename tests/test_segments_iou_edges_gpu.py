"""A13 segment fits and A16 rotated IoU on the inputs that seeded random scans and boxes never produce.

Segments: scans with PRESCRIBED segment lengths (every n from 3 to 28, the 64 / 128 / 256 boundaries of the
lane-strided loops, powers of two and odd / even n for the in-wave bitonic median, dropped segments between kept
ones, nothing kept), the fit columns of EVERY segment of three or more points against an np.longdouble solve under
a conditioning-scaled bound, the max_seg truncation contract of include/pof_abi.h, and runs of range exactly 0.
Rotated IoU: the pairs whose intersection is decided by an equality (identical, edge- and corner-sharing,
contained, zero-width boxes) bit for bit against the oracle, and both valid counts on a NaN-filled output.

The tests without the gpu mark are the preconditions of the fixtures (they need no device).
"""
import contextlib
import functools

import numpy as np
import pytest

from oracle import ref_numpy as R

DEV = "cuda"
INC = np.radians(0.5)
JUMP = 0.5
EPS = 2.0 ** -52
LEVELS = (2.0, 4.0, 6.0, 3.0, 5.0)      # neighbours differ by >= 1 m: every boundary is a cut at JUMP

LISTS = {
    450: (
        tuple(range(3, 29)) + (47,),                     # every n from 3 to 28 (sum 403) and the fill
        (30, 31, 32, 33, 63, 64, 65, 66, 66),
        (127, 128, 129, 66),
        (255, 192, 3),
        (256, 191, 3),
        (257, 190, 3),
        (1, 2, 3, 1, 1, 2, 4, 2, 1, 5, 428),             # dropped segments at index 0 and between kept ones
        (444, 3, 3),
        (450,),
        (2,) * 225,                                      # nothing kept
    ),
    451: ((65, 129, 257),),
    120: ((64, 33, 16, 7),),
}


def build_scan(lengths, N, seed=0):
    """float32 scan of N points whose jump-distance segments have exactly `lengths`.  Segment s sits on level
    LEVELS[s % 5] and takes shape s % 3: a straight wall lvl / cos(phi - phi_mid) (only up to 120 points at 0.5
    degrees: a wider wall jumps inside itself; longer ones become arcs), a shallow arc, or lvl + k / 256 with
    integer k in [-8, 8] -- exact in float32 and repeated, so both medians see ties."""
    assert sum(lengths) == N
    phi = R.laser_phi(INC, N)
    rng = np.random.default_rng(seed)
    r = np.empty(N)
    p0 = 0
    for s, n in enumerate(lengths):
        lvl, shape = LEVELS[s % 5], s % 3
        if shape == 0 and n <= 120:
            seg = lvl / np.cos(phi[p0:p0 + n] - 0.5 * (phi[p0] + phi[p0 + n - 1]))
        elif shape == 2:
            seg = lvl + rng.integers(-8, 9, n) / 256.0
        else:
            seg = lvl - 0.08 * np.sin(np.pi * (np.arange(n) + 0.5) / n)
        r[p0:p0 + n] = seg
        p0 += n
    return r.astype(np.float32)


def fixture_scans(N):
    return np.stack([build_scan(ls, N, seed=N + i) for i, ls in enumerate(LISTS[N])])


def lengths_of(cuts, N):
    return tuple(np.diff(np.concatenate(([0], cuts, [N]))).tolist())


def dropout_scan():
    """5 m scan with a 3-point run of range exactly 0 at index 0, a 6-point and a 2-point run of 0, and an
    ordinary 3-point segment."""
    r = np.full(450, 5.0, dtype=np.float32)
    r[0:3] = 0.0
    r[100:106] = 0.0
    r[200:202] = 0.0
    r[300:303] = 3.0
    return r


DROPOUT_LENGTHS = (3, 97, 6, 94, 2, 98, 3, 147)


def inf_scan():
    r = np.full(450, 5.0, dtype=np.float32)
    r[50:54] = np.inf
    return r


# ------------------------------------------------------------------ referee and CPU restatement of the fits
def referee(x, y):
    """np.longdouble solve of the formulas in the header of csrc/segment_lsq.hip on float64 points: mean, centred
    moments, k = Suv / Suu, b = my - k mx, the 2x2 circle solve [[Suu,Suv],[Suv,Svv]] (uc,vc) = (Suz,Svz) / 2,
    rc^2 = uc^2 + vc^2 + Sz / n, then Sc and the line residual from those.

    -> (values, units): values of k, b, xc, yc, rc, Sc, res, and for each the error a computation of unit
    round-off 2^-52 may make on THIS segment, up to a constant per column:
      k, b, xc, yc   cond 2^-52 max(|value|, 1),     cond = Suu Svv / (Suu Svv - Suv^2)
      rc             cond 2^-52 rc
      Sc  = sum t_i^2, t_i = rc - sqrt(d_i), d_i = |centre - p_i|:  dSc = sum 2 t_i (drc - dd_i / (2 sqrt(d_i))) and
          |dd_i| <= |dxc| + |dyc|, plus the round-off of the sum itself, so
          unit = sum 2 |t_i| (unit_rc + (unit_xc + unit_yc) / (2 sqrt(d_i))) + 2^-52 sum t_i^2
      res = (k / m) Sx - Sy / m - n |b| / m, m = sqrt(k^2 + 1):  d(k / m) / dk = 1 / m^3, d(1 / m) / dk = -k / m^3, so
          unit = (|Sx| + |k| (|Sy| + n |b|)) / m^3 unit_k + (n / m) unit_b + 2^-52 (|k Sx| + |Sy| + n |b|) / m
          (the three terms cancel to 0 whenever b < 0: only the sum of ABSOLUTE terms bounds the result)."""
    L = np.longdouble
    x, y = x.astype(L), y.astype(L)
    n = L(len(x))
    sx, sy = x.sum(), y.sum()
    mx, my = sx / n, sy / n
    u, v = x - mx, y - my
    z = u * u + v * v
    suu, svv, suv = (u * u).sum(), (v * v).sum(), (u * v).sum()
    suz, svz, sz = (u * z).sum(), (v * z).sum(), z.sum()
    k = suv / suu
    b = my - k * mx
    m = np.sqrt(k * k + 1)
    res = (k / m) * sx - sy / m - n * abs(b / m)
    det = suu * svv - suv * suv
    uc = (suz * svv - svz * suv) / det / 2
    vc = (svz * suu - suz * suv) / det / 2
    rc = np.sqrt(uc * uc + vc * vc + sz / n)
    xc, yc = uc + mx, vc + my
    d = np.sqrt((xc - x) ** 2 + (yc - y) ** 2)
    t = rc - np.sqrt(d)
    sc = (t * t).sum()
    e = (suu * svv / det) * L(EPS)
    unit = {c: e * max(abs(val), 1) for c, val in (("k", k), ("b", b), ("xc", xc), ("yc", yc))}
    unit["rc"] = e * rc
    unit["Sc"] = (2 * abs(t) * (unit["rc"] + (unit["xc"] + unit["yc"]) / (2 * np.sqrt(d)))).sum() + L(EPS) * sc
    unit["res"] = ((abs(sx) + abs(k) * (abs(sy) + n * abs(b))) / m ** 3 * unit["k"] + n / m * unit["b"]
                   + L(EPS) * (abs(k * sx) + abs(sy) + n * abs(b)) / m)
    return dict(k=k, b=b, xc=xc, yc=yc, rc=rc, Sc=sc, res=res), unit


def wave_sum(a):
    """The kernel's summation order: lane l of 64 adds elements l, l + 64, ... in turn, an xor tree closes."""
    acc = np.zeros(64)
    for row in np.concatenate([a, np.zeros(-len(a) % 64)]).reshape(-1, 64):
        acc = acc + row
    w = 64
    while w > 1:
        w //= 2
        acc = acc[:w] + acc[w:2 * w]
    return acc[0]


def restate64(x, y, total=wave_sum):
    """float64 restatement of the kernel's centred solve, statement by statement, sums taken by `total`."""
    n = float(len(x))
    sumx, sumy = total(x), total(y)
    mx, my = sumx / n, sumy / n
    u, v = x - mx, y - my
    z = u * u + v * v
    suu, svv, suv = total(u * u), total(v * v), total(u * v)
    suz, svz, sz = total(u * z), total(v * z), total(z)
    k = suv / suu
    b = my - k * mx
    nrm = np.sqrt(k * k + 1.0)
    res = (k / nrm) * sumx + (-1.0 / nrm) * sumy - n * abs(b / nrm)
    det = suu * svv - suv * suv
    uc = 0.5 * (suz * svv - svz * suv) / det
    vc = 0.5 * (svz * suu - suz * suv) / det
    rc = np.sqrt(uc * uc + vc * vc + sz / n)
    xc, yc = uc + mx, vc + my
    dx, dy = xc - x, yc - y
    t = rc - np.sqrt(np.sqrt(dx * dx + dy * dy))
    return dict(k=k, b=b, xc=xc, yc=yc, rc=rc, Sc=total(t * t), res=res)


FIT_COLS = ("k", "b", "xc", "yc", "rc", "Sc", "res")
PLAIN_COL = dict(res=5, Sc=6, rc=7, k=12, b=13, xc=14, yc=15)
REF_COL = dict(res=6, Sc=7, rc=8)


def segments_of(scan, cs):
    """[(start, x, y)] of every segment of three or more points, points as the kernel forms them."""
    r = scan.astype(np.float64)
    x, y = r * cs[:, 0], r * cs[:, 1]
    edges = np.concatenate(([0], R.segment_cuts(scan, JUMP), [len(scan)]))
    return [(s, p0, x[p0:p1], y[p0:p1]) for s, (p0, p1) in enumerate(zip(edges[:-1], edges[1:])) if p1 - p0 >= 3]


def ratios(values, want, unit):
    return {c: float(abs(np.longdouble(values[c]) - want[c]) / unit[c]) for c in FIT_COLS}


@contextlib.contextmanager
def oracle_on(cs):
    """Run the oracle on the kernel's own points: the device cos / sin table is within 1 ulp of libm
    (test_phi_table), and one ulp of a point moves the curvature of a float32-straight wall by more than the
    1e-9 bar; with the same points the oracle's per-point arithmetic is the kernel's operation for operation."""
    orig = R.polar_to_xy
    R.polar_to_xy = lambda r, phi: (r * cs[:, 0], r * cs[:, 1])
    try:
        yield
    finally:
        R.polar_to_xy = orig


# ------------------------------------------------------------------ preconditions (no device)
@pytest.mark.parametrize("N", sorted(LISTS))
def test_fixture_has_prescribed_lengths(N):
    for ls, scan in zip(LISTS[N], fixture_scans(N)):
        assert lengths_of(R.segment_cuts(scan, JUMP), N) == ls
    if N == 450:
        assert lengths_of(R.segment_cuts(dropout_scan(), JUMP), 450) == DROPOUT_LENGTHS
        with np.errstate(invalid="ignore"):
            assert lengths_of(R.segment_cuts(inf_scan(), JUMP), 450) == (50, 4, 396)


def test_fixture_ties_and_conditioning():
    """The quantised segments repeat values (ties for both medians), and the wall segments are the
    ill-conditioned circle fits the scaled bound has to carry."""
    phi = R.laser_phi(INC, 450)
    cs = np.stack([np.cos(phi), np.sin(phi)], axis=1)
    scans = fixture_scans(450)
    assert len(np.unique(scans[1][61:93])) < 32          # segment 2 of the second list: 32 quantised points
    conds = []
    for scan in scans:
        for _, _, x, y in segments_of(scan, cs):
            want, unit = referee(x, y)
            conds.append(float(unit["rc"] / want["rc"] / EPS))
    conds = np.array(conds)
    assert (conds > 1e6).mean() > 0.2 and (conds < 1e3).sum() > 10


def test_oracle_on_zero_runs():
    """What the reference's pinv gives on coincident points (the kernel has to match it): finite zeros in every
    fit column, NaN only in curvature and angle."""
    phi = R.laser_phi(INC, 450)
    with np.errstate(all="ignore"):
        cuts, feat = R.segment_features(dropout_scan(), phi, JUMP)
    for s, n in ((0, 3), (2, 6)):
        assert feat[s, 0] == n
        assert np.array_equal(feat[s, [5, 6, 7, 12, 13, 14, 15]], np.zeros(7))
        assert np.isnan(feat[s, [10, 11]]).all()
    assert feat[4, 0] == 2 and np.isnan(feat[4, [5, 6, 7, 10, 11, 12, 13, 14, 15]]).all()


def iou_boxes():
    """Twelve 2-D boxes [x, y, l, w, rot] whose pairs branch on equality inside inter_area."""
    return np.array([
        [0, 0, 1, 1, 0], [0, 0, 1, 1, np.pi / 2], [0, 0, 1, 1, np.pi], [0, 0, 1, 1, 1e-4],
        [1, 0, 1, 1, 0],                  # shares an edge with the unit square
        [1, 1, 1, 1, 0],                  # shares a corner
        [0.25, 0, 1, 1, 0],
        [0, 0, 0.5, 0.5, 0.3],            # contained
        [0, 0, 2, 0.5, np.pi / 4],
        [0, 0, 0, 1, 0],                  # zero width
        [0, 0, 0, 0, 0],                  # zero area
        [1e4, 1e4, 1, 1, 0],
    ], dtype=np.float32)


ZERO_AREA = (9, 10)


def iou_boxes_3d(z, h=1.5):
    """The same boxes in the reference's 3-D column order x, y, z, l, w, h, rot."""
    b = iou_boxes()
    out = np.zeros((len(b), 7), dtype=np.float32)
    out[:, [0, 1, 3, 4, 6]] = b
    out[:, 2], out[:, 5] = z, h
    return out


@functools.lru_cache(maxsize=None)
def iou_oracle(form, crit):
    """form 0: 2-D, 1: 3-D with equal z and h, 2: 3-D with |dz| = h exactly (the zero-height branch)."""
    if form == 0:
        return R.rotate_iou(iou_boxes(), iou_boxes(), criterion=crit)
    return R.rotate_iou(iou_boxes_3d(0.0), iou_boxes_3d(0.0 if form == 1 else 1.5), criterion=crit, is_3d=True)


def test_oracle_on_degenerate_boxes():
    """NaN / inf in the oracle only on pairs with a zero-area box; criterion 2 (the bare intersection) finite."""
    zero = np.zeros((12, 12), dtype=bool)
    zero[list(ZERO_AREA), :] = True
    zero[:, list(ZERO_AREA)] = True
    for crit in (-1, 0, 1, 2):
        want = iou_oracle(0, crit)
        assert np.isfinite(want[~zero]).all()
        if crit == 2:
            assert np.isfinite(want).all()
    want = iou_oracle(0, -1)
    assert want[0, 0] == 1.0 and want[0, 4] == 0.0 and want[0, 5] == 0.0 and want[0, 11] == 0.0
    assert 0.0 < want[0, 6] < 1.0 and 0.0 < want[0, 7] < 1.0
    assert np.array_equal(iou_oracle(2, 2), np.zeros((12, 12), dtype=np.float32))


# ------------------------------------------------------------------ device side
def T(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def ops():
    import torch
    from planar_optical_flow_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _ops


def run_scans(ops, scans, max_seg=None):
    """Both entry points on one batch -> dict of NumPy arrays (and the kernel's cos / sin table)."""
    N = scans.shape[1]
    tab = ops.phi_table(INC, N)
    nxt = scans + np.float32(0.01)
    dt = np.linspace(0.05, 0.2, len(scans))
    sid, num, feat = ops.segment_features(T(scans), tab, JUMP, max_seg=max_seg)
    sid2, num2, kept, ref, plain = ops.segment_features_reference(T(scans), tab, T(nxt), T(dt), jump_dist=JUMP,
                                                                  max_seg=max_seg, want_plain=True)
    out = dict(sid=sid, num=num, feat=feat, sid2=sid2, num2=num2, kept=kept, ref=ref, plain=plain)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out.update(cs=tab[N:].cpu().numpy().reshape(N, 2), nxt=nxt, dt=dt, scans=scans)
    return out


def oracle_rows(run, b):
    """(plain [S,16], reference rows [K,15]) of scan b by the oracle, on the kernel's points."""
    scan, N = run["scans"][b], run["scans"].shape[1]
    phi = R.laser_phi(INC, N)
    with oracle_on(run["cs"]), np.errstate(all="ignore"):
        _, plain = R.segment_features(scan, phi, JUMP)
        rows = R.compute_feature_reference(scan.astype(np.float64), phi, [], run["nxt"][b].astype(np.float64), 0.0,
                                           run["dt"][b], jump_dist=JUMP)
    return plain, rows


@pytest.fixture(scope="module")
def runs(ops):
    """Kernel outputs and oracle rows of the three fixture batches, computed once."""
    out = {}
    for N in LISTS:
        run = run_scans(ops, fixture_scans(N))
        run["oracle"] = [oracle_rows(run, b) for b in range(len(LISTS[N]))]
        out[N] = run
    return out


def kept_of(lengths):
    return [s for s, n in enumerate(lengths) if n > 2]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.gpu
def test_fit_columns_vs_longdouble_referee(runs):
    """Plain columns 5, 6, 7, 12-15 and reference-row columns 6, 7, 8 of EVERY segment of three or more points
    (walls included, no mask) within c_col * unit(segment) of the np.longdouble referee, unit as derived in
    referee().  c_col is not chosen: it is 4 x the largest error / unit that the float64 restatement of the same
    solve, summed in the kernel's order, makes over this fixture (the 4 covers the device sqrt and divide).
    Prints both the restatement's and the kernel's largest ratio per column."""
    segs = []
    for N, run in runs.items():
        for bi, ls in enumerate(LISTS[N]):
            kq = {s: q for q, s in enumerate(kept_of(ls))}
            for s, p0, x, y in segments_of(run["scans"][bi], run["cs"]):
                assert len(x) == ls[s]
                want, unit = referee(x, y)
                got = {c: run["feat"][bi, s, PLAIN_COL[c]] for c in FIT_COLS}
                for c, col in REF_COL.items():
                    assert run["ref"][bi, kq[s], col] == got[c] or np.isnan(got[c]), (N, bi, s, c)
                segs.append(((N, bi, s, len(x)), ratios(restate64(x, y), want, unit),
                             ratios(restate64(x, y, np.sum), want, unit), ratios(got, want, unit)))
    assert len(segs) == 64
    worst = {}
    for c in FIT_COLS:
        r64 = max(s[1][c] for s in segs)
        rnp = max(s[2][c] for s in segs)
        at, _, _, rk = max(segs, key=lambda s: s[3][c] if np.isfinite(s[3][c]) else np.inf)
        worst[c] = (rk[c], 4.0 * r64, at)
        print("fit column %-3s largest error / unit: restatement %.3g (NumPy order %.3g), kernel %.3g at "
              "(N, scan, segment, n) = %s" % (c, r64, rnp, rk[c], at))
    for c, (rk, bound, at) in worst.items():
        assert rk <= bound, "column %s: kernel error %.3g units > 4 x restatement %.3g at %s" % (c, rk, bound, at)


def _assert_close(got, want, where, rtol=1e-9, atol=1e-12):
    assert np.array_equal(np.isnan(got), np.isnan(want)), where
    ok = ~np.isnan(want)
    ratio = np.zeros(want.shape)
    ratio[ok] = np.abs(got[ok] - want[ok]) / (atol + rtol * np.abs(want[ok]))
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert ratio[at] <= 1.0, "%s: error / tolerance %.3g at %s (got %r, want %r)" % (where, ratio[at], at, got[at], want[at])
    return ratio[at]


@pytest.mark.gpu
def test_curvature_and_angle_every_segment(runs):
    """Summed curvature and mean angular difference (plain 10, 11; reference rows 11, 12) of every segment of
    three or more points against the oracle -- same float64 operations per triple, so the no-fit bar 1e-9 /
    1e-12 holds on the shortest segments and on float32-straight walls alike -- and the other no-fit columns."""
    worst = 0.0
    for N, run in runs.items():
        for bi, ls in enumerate(LISTS[N]):
            plain, rows = run["oracle"][bi]
            S, K = len(ls), len(kept_of(ls))
            assert plain.shape == (S, 16) and rows.shape == (K, 15)
            n3 = np.array(ls) >= 3
            assert not np.isnan(plain[n3][:, [10, 11]]).any()
            worst = max(worst, _assert_close(run["feat"][bi, :S][:, [10, 11]], plain[:, [10, 11]], (N, bi, "plain 10 11")))
            _assert_close(run["feat"][bi, :S][:, [1, 2, 3, 4, 8, 9]], plain[:, [1, 2, 3, 4, 8, 9]], (N, bi, "plain"))
            if K:
                worst = max(worst, _assert_close(run["ref"][bi, :K][:, [11, 12]], rows[:, [11, 12]], (N, bi, "ref 11 12")))
                _assert_close(run["ref"][bi, :K][:, [1, 3, 4, 5, 9, 10, 13]], rows[:, [1, 3, 4, 5, 9, 10, 13]], (N, bi, "ref"))
    print("curvature / angle: largest error / tolerance %.3g" % worst)


@pytest.mark.gpu
def test_lengths_medians_seg_id(runs):
    """Sizes, counts and seg_id exact on every fixture scan; the median deviation (reference column 2) against
    np.median of the float64 points at 1e-12 for every n of the lists, ties included; column 4 NaN exactly where
    the oracle's is; nothing kept leaves the NaN fill; the plain table of the _ex call is the plain call's."""
    for N, run in runs.items():
        assert np.array_equal(run["sid"], run["sid2"]) and np.array_equal(run["num"], run["num2"])
        assert same_bits(run["feat"], run["plain"])
        for bi, ls in enumerate(LISTS[N]):
            S, kept = len(ls), kept_of(ls)
            K = len(kept)
            assert run["num"][bi] == S and run["kept"][bi] == K
            assert np.array_equal(run["sid"][bi], np.repeat(np.arange(S), ls))
            assert np.array_equal(run["feat"][bi, :S, 0], np.array(ls, dtype=np.float64))
            assert np.isnan(run["feat"][bi, S:]).all() and np.isnan(run["ref"][bi, K:]).all()
            assert np.array_equal(run["ref"][bi, :K, 0], np.array([ls[s] for s in kept], dtype=np.float64))
            rows = run["oracle"][bi][1]
            assert np.array_equal(np.isnan(run["ref"][bi, :K, 4]), np.isnan(rows[:, 4]))
            assert np.isnan(rows[:, 4]).any() == (0 < K < 4)
            r = run["scans"][bi].astype(np.float64)
            xy = np.stack([r * run["cs"][:, 0], r * run["cs"][:, 1]], axis=1)
            starts = np.concatenate(([0], np.cumsum(ls)))
            for q, s in enumerate(kept):
                seg = xy[starts[s]:starts[s + 1]]
                want = np.linalg.norm(seg - np.median(seg, axis=0)) / len(seg)
                np.testing.assert_allclose(run["ref"][bi, q, 2], want, rtol=1e-12, atol=0, err_msg=str((N, bi, s, ls[s])))
    assert runs[450]["kept"][9] == 0 and runs[450]["kept"][8] == 1


@pytest.mark.gpu
def test_max_seg_truncation(ops, runs):
    """max_seg below the number of segments (include/pof_abi.h, A13): num_seg and seg_id are those of the whole
    scan, plain rows [0, max_seg) are bit for bit the untruncated call's, num_kept counts the kept segments among
    the first max_seg, the reference rows are those of a kept list cut there (column 4 NaN where kept[min(q+1, 3)]
    no longer exists), and nothing is written past row max_seg of either table.  A batch of scans with other cut
    positions, large enough to reach every compute unit, runs before every truncated launch, so that a segment
    start left in LDS by an earlier launch of the same scan cannot stand in for one the kernel failed to write."""
    import torch
    from planar_optical_flow_amd import _lib
    ls = LISTS[450][0]
    scan = fixture_scans(450)[:1]
    other = T(np.repeat(fixture_scans(450)[9:10], 1024, axis=0))
    full = runs[450]
    S, kept = len(ls), kept_of(ls)
    rows = full["oracle"][0][1]
    tab = ops.phi_table(INC, 450)
    SENT = -777.0
    for m in (S, S - 1, 5, 1):
        ops.segment_features(other, tab, JUMP, max_seg=226)
        run = run_scans(ops, scan, max_seg=m)
        Kt = sum(1 for s in kept if s < m)
        assert run["num"][0] == S and run["num2"][0] == S and run["kept"][0] == Kt
        assert np.array_equal(run["sid"][0], full["sid"][0]) and np.array_equal(run["sid2"][0], full["sid"][0])
        assert run["feat"].shape == (1, m, 16) and run["ref"].shape == (1, m, 15)
        assert same_bits(run["feat"][0], full["feat"][0, :m]) and same_bits(run["plain"][0], full["feat"][0, :m])
        want = full["ref"][0, :Kt].copy()
        cut = np.minimum(np.arange(Kt) + 1, 3) >= Kt
        want[cut, 4] = np.nan
        assert same_bits(run["ref"][0, :Kt], want), m
        assert np.isnan(run["ref"][0, Kt:]).all()
        oracle = rows[:Kt].copy()
        oracle[cut, 4] = np.nan
        _assert_close(run["ref"][0, :Kt][:, [1, 2, 3, 4, 5, 9, 10, 13]], oracle[:, [1, 2, 3, 4, 5, 9, 10, 13]], ("max_seg", m))
        # the C entry point on tables two rows longer than max_seg, prefilled
        ops.segment_features(other, tab, JUMP, max_seg=226)
        feat = torch.full((m + 2, 16), SENT, dtype=torch.float64, device=DEV)
        ref = torch.full((m + 2, 15), SENT, dtype=torch.float64, device=DEV)
        sid = torch.empty(450, dtype=torch.int32, device=DEV)
        num = torch.empty(1, dtype=torch.int32, device=DEV)
        nk = torch.empty(1, dtype=torch.int32, device=DEV)
        r, nx, dt = T(scan), T(run["nxt"]), T(run["dt"])
        _lib.call("pof_segment_features_ex", ops._ptr(r), ops._ptr(nx), ops._ptr(tab), 1, 450, JUMP, ops._ptr(dt),
                  None, None, 0.5, m, ops._ptr(sid), ops._ptr(num), ops._ptr(nk), ops._ptr(feat), ops._ptr(ref),
                  ops._stream())
        feat, ref = feat.cpu().numpy(), ref.cpu().numpy()
        assert num.item() == S and nk.item() == Kt and np.array_equal(sid.cpu().numpy(), full["sid"][0])
        assert same_bits(feat[:m], full["feat"][0, :m]) and same_bits(ref[:Kt], want)
        assert np.all(feat[m:] == SENT) and np.all(ref[Kt:] == SENT), "write past row max_seg = %d" % m


@pytest.mark.gpu
def test_zero_range_runs(ops):
    """Runs of range exactly 0 are coincident points: the normal equations are singular and the reference's pinv
    returns the minimum-norm solution, 0 for k, b, xc, yc, radius, Sc and the residual (NaN only in curvature and
    angle).  Every column of every segment against the oracle, NaN class included; the fit columns of the zero
    runs exactly, the others at the oracle's own accuracy (an uncentred float64 pinv: 1e-6 / 1e-9, the suite's
    bar for k and b)."""
    scans = dropout_scan()[None]
    run = run_scans(ops, scans)
    plain, rows = oracle_rows(run, 0)
    S = len(DROPOUT_LENGTHS)
    kept = kept_of(DROPOUT_LENGTHS)
    assert run["num"][0] == S and run["kept"][0] == len(kept) == 7
    assert np.array_equal(run["sid"][0], np.repeat(np.arange(S), DROPOUT_LENGTHS))
    got, gref = run["feat"][0, :S], run["ref"][0, :len(kept)]
    assert same_bits(run["feat"], run["plain"])
    assert np.array_equal(np.isnan(got), np.isnan(plain)), np.argwhere(np.isnan(got) != np.isnan(plain))
    assert np.array_equal(np.isnan(gref), np.isnan(rows)), np.argwhere(np.isnan(gref) != np.isnan(rows))
    fit, nofit = [5, 6, 7, 12, 13, 14, 15], [0, 1, 2, 3, 4, 8, 9, 10, 11]
    for s in (0, 2):
        assert np.array_equal(got[s, fit], np.zeros(7)) and np.array_equal(plain[s, fit], np.zeros(7))
        assert np.array_equal(gref[kept.index(s), [6, 7, 8]], np.zeros(3))
    assert np.isnan(got[4, fit]).all()
    _assert_close(got[:, nofit], plain[:, nofit], "plain")
    _assert_close(got[:, fit], plain[:, fit], "plain fits", rtol=1e-6, atol=1e-9)
    _assert_close(gref[:, [0, 1, 2, 3, 4, 5, 9, 10, 11, 12, 13, 14]], rows[:, [0, 1, 2, 3, 4, 5, 9, 10, 11, 12, 13, 14]], "ref")
    _assert_close(gref[:, [6, 7, 8]], rows[:, [6, 7, 8]], "ref fits", rtol=1e-6, atol=1e-9)


@pytest.mark.gpu
def test_inf_run_cuts_and_sizes(ops):
    """Four consecutive inf: |inf - inf| is NaN and cuts nothing, so they form one segment.  Only what needs no
    fit is checked (the oracle's pinv does not return on a segment that holds inf)."""
    scan = inf_scan()
    with np.errstate(invalid="ignore"):
        cuts = R.segment_cuts(scan, JUMP)
    ls = lengths_of(cuts, 450)
    run = run_scans(ops, scan[None])
    for sid, num, feat in ((run["sid"], run["num"], run["feat"]), (run["sid2"], run["num2"], run["plain"])):
        assert num[0] == len(ls) and np.array_equal(sid[0], np.repeat(np.arange(len(ls)), ls))
        assert np.array_equal(feat[0, :len(ls), 0], np.array(ls, dtype=np.float64))
    assert run["kept"][0] == 3 and np.array_equal(run["ref"][0, :3, 0], np.array(ls, dtype=np.float64))


@pytest.mark.gpu
def test_rotate_iou_degenerate_pairs(ops):
    """All 12 x 12 pairs of iou_boxes(), every criterion, 2-D, 3-D with equal z and h, and 3-D with |dz| = h
    exactly: bit-identical to the oracle (float32 in the reference's operation order), NaN / inf only where the
    oracle has them."""
    forms = ((iou_boxes(), iou_boxes(), False), (iou_boxes_3d(0.0), iou_boxes_3d(0.0), True),
             (iou_boxes_3d(0.0), iou_boxes_3d(1.5), True))
    for form, (bx, qx, is3d) in enumerate(forms):
        for crit in (-1, 0, 1, 2):
            got = ops.rotate_iou(T(bx), T(qx), criterion=crit, is_3d=is3d).cpu().numpy()
            want = iou_oracle(form, crit)
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
            diff = np.argwhere((got.view(np.int32) != want.view(np.int32)) & ~np.isnan(want))
            assert len(diff) == 0, (form, crit, diff[:8].tolist(), got[tuple(diff[0])], want[tuple(diff[0])])


@pytest.mark.gpu
def test_rotate_iou_valid_counts(ops):
    """G = 5 groups of 7 x 11 pairs (one full wave and 13 lanes per group), n_valid and k_valid together and each
    alone, 2-D and 3-D, through the C entry point on an output prefilled with NaN: entries inside both counts
    equal the per-group oracle, every entry outside is written and is exactly 0."""
    import torch
    from planar_optical_flow_amd import _lib
    G, N, K = 5, 7, 11
    rng = np.random.default_rng(16)

    def boxes(n, s):                                     # centres close, sizes large: every pair overlaps
        b = np.zeros((G, n, s), dtype=np.float32)
        b[..., :2] = rng.uniform(-0.2, 0.2, (G, n, 2))
        if s == 5:
            b[..., 2:4] = rng.uniform(0.8, 1.5, (G, n, 2))
            b[..., 4] = rng.uniform(-np.pi, np.pi, (G, n))
        else:
            b[..., 2] = rng.uniform(-0.2, 0.2, (G, n))
            b[..., 3:6] = rng.uniform(0.8, 1.5, (G, n, 3))
            b[..., 6] = rng.uniform(-np.pi, np.pi, (G, n))
        return b

    nv = np.array([7, 0, 3, 7, 1], dtype=np.int32)
    kv = np.array([11, 4, 0, 11, 1], dtype=np.int32)
    for s, is3d in ((5, False), (7, True)):
        bx, qx = boxes(N, s), boxes(K, s)
        want = np.stack([R.rotate_iou(bx[g], qx[g], is_3d=is3d) for g in range(G)])
        assert (want > 0).all()
        perm = [0, 1, 3, 4, 6, 2, 5] if is3d else list(range(5))
        db, dq = T(bx[..., perm]), T(qx[..., perm])
        for use_n, use_k in ((True, True), (True, False), (False, True)):
            out = torch.full((G, N, K), float("nan"), dtype=torch.float32, device=DEV)
            dn, dk = T(nv), T(kv)
            _lib.call("pof_rotate_iou", ops._ptr(db), ops._ptr(dq), ops._ptr(out), G, N, K,
                      ops._ptr(dn) if use_n else None, ops._ptr(dk) if use_k else None, -1, int(is3d), ops._stream())
            got = out.cpu().numpy()
            for g in range(G):
                n, k = (nv[g] if use_n else N), (kv[g] if use_k else K)
                assert np.array_equal(got[g, :n, :k], want[g, :n, :k]), (s, use_n, use_k, g)
                mask = np.ones((N, K), dtype=bool)
                mask[:n, :k] = False
                assert np.all(got[g][mask] == 0.0), (s, use_n, use_k, g)
