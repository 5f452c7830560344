"""Scan-to-scan matching (pof_scan_match, N8) without a GPU: ``match_oracle`` is the float64 NumPy restatement of the
header comment in include/pof_abi.h, run here on seeded polygon rooms that are ray-cast from two poses -- the result has
to invert get_displacement_from_odometry (src/utils/utils.py:639-662), i.e. equal ``true_motion`` of the pose pair -- and
the host-side argument checks.  tests/test_scan_match_gpu.py imports the helpers below.

Bounds against the true motion (``motion_error`` of tests/test_ego_motion.py, metres): fixed from the restatement's own
results on the committed seeds (printed by the tests; the worst is quoted next to each constant) with a factor 2 margin,
and in any case 1/10 of the step.
Device against oracle (``tolerance``): the two differ in the order of their sums and in the last bit of sincos, so the
tolerance is 100 x the largest disagreement between the oracle's own pairwise and sequential evaluations on the inputs
at hand, at least 1e-13 and asserted to stay below 1e-10.  The algorithm takes discrete decisions (which vertex is
nearest, inside the gate or not, which line partner, the rounding of the beam shift, the Huber threshold, a gap at its
limit, the early exit, a pivot at its floor); the oracle returns the smallest margin by which each kind was taken and the
committed cases are asserted to keep every one >= 1e-10, so that a reordering of sums cannot flip a decision."""
import inspect

import numpy as np
import pytest

from oracle import ref_numpy as R
from test_ego_motion import motion_error, seq_sum, true_motion

MARGIN_MIN = 1e-10
DEFAULTS = dict(max_range=20.0, window=16, gate=0.5, max_gap=0.3, huber_delta=0.05, iters=16, eps_theta=1e-7,
                eps_u=1e-7, min_pivot=1e-6)
# worst motion_error of the restatement on the committed scenes (printed by the tests), times 2
BOUND_CLEAN = 2 * 2.92e-4           # no noise, 8 rooms: 9.0e-6 to 2.92e-4 m, 3-4 iterations
BOUND_NOISE = 2 * 4.85e-3           # 1 cm range noise: up to 4.84e-3 m
BOUND_NOISE_BIG = 2 * 6.70e-3       # 1 cm range noise, steps four times larger: up to 6.69e-3 m
# iterations: 4 at most without noise (x 1.5); under noise the matches of a few points can alternate at the 1e-7 exit, so
# some scenes run all 16
ITERS_CLEAN, ITERS_NOISE, ITERS_NOISE_BIG = 6, 16, 16


# ---------------------------------------------------------------- scenes: a polygon room, ray-cast
def angle_table(N, angle_inc=np.radians(0.5)):
    """The [3N] table phi | (cos, sin) interleaved, as ops.phi_table lays it out, from NumPy."""
    phi = R.laser_phi(angle_inc, N)
    return np.concatenate([phi, np.stack([np.cos(phi), np.sin(phi)], axis=1).reshape(-1)])


def make_room(rng):
    """Segments [M,2,2]: an outer rectangle and three to five boxes that keep clear of the middle, where the sensor is."""
    hx, hy = rng.uniform(4, 8), rng.uniform(3, 6)
    rect = lambda cx, cy, a, b: [((cx - a, cy - b), (cx + a, cy - b)), ((cx + a, cy - b), (cx + a, cy + b)),
                                 ((cx + a, cy + b), (cx - a, cy + b)), ((cx - a, cy + b), (cx - a, cy - b))]
    segs = rect(0.0, 0.0, hx, hy)
    for _ in range(rng.integers(3, 6)):
        a, b = rng.uniform(0.25, 0.75, 2)
        while True:
            cx, cy = rng.uniform(-hx + 1, hx - 1), rng.uniform(-hy + 1, hy - 1)
            if np.hypot(cx, cy) > 2.2:
                break
        segs += rect(cx, cy, a, b)
    return np.asarray(segs, np.float64)


def ray_cast(segs, pose, phi):
    """Ranges [N] float64 of the beams pose[2] + phi from (pose[0], pose[1]) to the nearest segment (inf without one)."""
    ang = pose[2] + phi
    d = np.stack([np.cos(ang), np.sin(ang)], axis=1)[:, None]           # [N,1,2]
    p, e = segs[None, :, 0] - np.asarray(pose[:2]), (segs[:, 1] - segs[:, 0])[None]
    cross = lambda a, b: a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        den = cross(d, e)
        t, s = cross(p, e) / den, cross(p, d) / den
    t = np.where((den != 0) & (t > 0) & (s >= 0) & (s <= 1), t, np.inf)
    return t.min(axis=1)


def room_pairs(n, seed=5, N=450, noise=0.0, scale=1.0, angle_inc=np.radians(0.5)):
    """n seeded scan pairs -> list of (r_prev, r_cur float32 [N], true (theta, u), step length in motion_error units).
    The pose step is that of robust_cases (tests/test_ego_motion.py), +-0.05 m and +-0.03 rad, times `scale`."""
    rng = np.random.default_rng(seed)
    phi = R.laser_phi(angle_inc, N)
    out = []
    for _ in range(n):
        segs = make_room(rng)
        odom0 = np.concatenate([rng.uniform(-0.5, 0.5, 2), rng.uniform(-np.pi, np.pi, 1)])
        odom1 = odom0 + scale * np.concatenate([rng.uniform(-0.05, 0.05, 2), rng.uniform(-0.03, 0.03, 1)])
        r0, r1 = (ray_cast(segs, o, phi) + rng.normal(0, 1.0, N) * noise for o in (odom0, odom1))
        true = true_motion(odom0, odom1)[0]
        out.append((r0.astype(np.float32), r1.astype(np.float32), true, motion_error(true, np.zeros(3))))
    return out


def trajectory(T, B, seed=9, N=450, noise=0.0):
    """T scans of B sensors, each in a room of its own -> (scans float32 [T,B,N], poses [T,B,3])."""
    rng = np.random.default_rng(seed)
    phi = R.laser_phi(num_pts=N)
    scans, poses = np.zeros((T, B, N), np.float32), np.zeros((T, B, 3))
    for b in range(B):
        segs = make_room(rng)
        pose = np.concatenate([rng.uniform(-0.5, 0.5, 2), rng.uniform(-np.pi, np.pi, 1)])
        for t in range(T):
            poses[t, b] = pose
            scans[t, b] = (ray_cast(segs, pose, phi) + rng.normal(0, 1.0, N) * noise).astype(np.float32)
            pose = pose + np.concatenate([rng.uniform(-0.05, 0.05, 2), rng.uniform(-0.03, 0.03, 1)])
    return scans, poses


def add_people(r_cur, rng, share=0.2, width=15):
    """Pull `share` of the beams, in runs of `width`, 0.3-1.5 m towards the sensor, as people in front of the walls
    that moved in since the previous scan.  -> (ranges float32, instance ids [N] int32, num, det_cls [N] float64): one
    detection per run with a confident score, and one more run that is only a low-score detection on a wall."""
    N = len(r_cur)
    r = r_cur.astype(np.float64).copy()
    inst, det_cls = np.zeros(N, np.int32), np.zeros(N)
    runs = int(share * N) // width
    starts = rng.choice(N // width - 1, runs + 1, replace=False) * width
    for k, s in enumerate(starts[:runs]):
        r[s:s + width] = np.maximum(r[s:s + width] - rng.uniform(0.3, 1.5), 0.3)
        inst[s:s + width] = k + 1
        det_cls[k] = rng.uniform(0.6, 1.0)
    inst[starts[runs]:starts[runs] + width] = runs + 1
    det_cls[runs] = 0.2                                         # below the threshold: these wall points vote
    return r.astype(np.float32), inst, runs + 1, det_cls


def person_points(inst, num, det_cls, cls_thresh=0.5):
    """bool [N]: the points pof_scan_match leaves out (ids 1..clamp(num, 0, N) with det_cls >= cls_thresh)."""
    n = len(inst)
    nd = min(max(int(num), 0), n)
    ids = np.asarray(inst, np.int64)
    member = (ids >= 1) & (ids <= nd)
    person = np.zeros(n, bool)
    person[member] = np.asarray(det_cls)[ids[member] - 1] >= cls_thresh
    return person


# ---------------------------------------------------------------- restatement of the device arithmetic, one pair
def _beam_shift(th, dphi, N):
    if dphi == 0.0:
        return 0, np.inf
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q = np.float64(th) / np.float64(dphi)
        t = np.rint(q)
    if not t >= -N:
        t = -N
    if not t <= N:
        t = N
    margin = abs(abs(q - np.floor(q)) - 0.5) if np.isfinite(q) else np.inf
    return int(t), margin


class _Margins(dict):
    def take(self, kind, values):
        v = np.asarray(values, np.float64).reshape(-1)
        v = v[np.isfinite(v)]
        self["decisions"] = self.get("decisions", 0) + v.size
        if v.size:
            self[kind] = min(self.get(kind, np.inf), float(v.min()))


def _shift_centres(dphi, N):
    """N8's window centres: beam i + shift(th)."""
    def centres(qx, qy, th, valid, margins):
        shift, m_shift = _beam_shift(th, dphi, N)
        margins.take("shift", [m_shift])
        return np.arange(N) + shift
    return centres


def _correspond(ax, ay, px, py, valid, th, ux, uy, centres, W, gate2, gap2, margins):
    """The correspondence of every current point at (th, u) -> matched [N] bool, j [N], q, d, n [N,2] each.
    centres(qx, qy, th, valid, margins) -> mid [N] int: the centre of every point's search window."""
    N = len(ax)
    c, s = np.cos(th), np.sin(th)
    with np.errstate(invalid="ignore", over="ignore"):
        qx, qy = (c * px - s * py) + ux, (s * px + c * py) + uy
        mid = centres(qx, qy, th, valid, margins)
        i = np.arange(N)
        js = mid[:, None] + np.arange(-W, W + 1)[None]
        inside = (js >= 0) & (js < N)
        jc = np.where(inside, js, 0)
        assert jc.min() >= 0 and jc.max() < N                  # nothing outside [0, N) is read
        dx, dy = qx[:, None] - np.take(ax, jc, mode="raise"), qy[:, None] - np.take(ay, jc, mode="raise")
        d2 = dx * dx + dy * dy
        d2 = np.where(inside & ~np.isnan(d2), d2, np.inf)
        col = np.argmin(d2, axis=1)                            # the first minimum: the lower j
        bd, j = d2[i, col], jc[i, col]
        near = valid & (bd < np.inf) & (bd <= gate2)
        second = np.partition(d2, 1, axis=1)[:, 1]
        margins.take("nearest", (second - bd)[near])
        margins.take("gate", np.abs(bd - gate2)[valid & (bd < np.inf)])
        jx, jy = ax[j], ay[j]
        qual, g2, e, f2s = [], [], [], []
        for side in (-1, 1):
            kk = j + side
            ok = near & (kk >= 0) & (kk < N)
            kc = np.where(ok, kk, 0)
            fx, fy = ax[kc] - jx, ay[kc] - jy
            f2 = fx * fx + fy * fy
            qual.append(ok & (f2 > 0.0) & (f2 <= gap2))        # NaN: not valid
            margins.take("gap", np.abs(f2 - gap2)[ok & (f2 > 0.0)])
            gx, gy = qx - ax[kc], qy - ay[kc]
            g2.append(gx * gx + gy * gy)
            e.append((fx, fy))
            f2s.append(f2)
        plus = qual[1] & (~qual[0] | (g2[1] < g2[0]))
        margins.take("partner", np.abs(g2[1] - g2[0])[qual[0] & qual[1]])
        matched = near & (qual[0] | qual[1])
        ex, ey = np.where(plus, e[1][0], e[0][0]), np.where(plus, e[1][1], e[0][1])
        length = np.sqrt(np.where(plus, f2s[1], f2s[0]))
        with np.errstate(divide="ignore"):
            nx, ny = -ey / length, ex / length
        return matched, j, (qx, qy), (qx - jx, qy - jy), (nx, ny)


def _iterate(ax, ay, px, py, valid, init, centres, window, gate, max_gap, huber_delta, iters, eps_theta, eps_u,
             min_pivot, sum, margins):
    """The matcher core from the start value init [3]: the iterations and the final correspondence pass, around the
    window centres of ``_correspond``.  -> failed, (theta, u) [3], count, rms, iters_used, obs, corr [N],
    flow_residual [N,2]."""
    N = len(ax)
    th, ux, uy = (float(v) for v in init)
    gate2, gap2 = gate * gate, max_gap * max_gap
    failed, used, count, rms, obs = False, 0, 0, np.nan, 0.0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for it in range(int(iters)):
            k, _, (qx, qy), (dx, dy), (nx, ny) = _correspond(ax, ay, px, py, valid, th, ux, uy, centres, window,
                                                               gate2, gap2, margins)
            qx, qy, dx, dy, nx, ny = (v[k] for v in (qx, qy, dx, dy, nx, ny))
            r = nx * dx + ny * dy
            ar = np.abs(r)
            if huber_delta > 0.0:
                w = np.where(ar > huber_delta, huber_delta / ar, 1.0)
                margins.take("huber", np.abs(ar - huber_delta))
            else:
                w = np.ones_like(r)
            J = (nx * (-qy) + ny * qx, nx, ny)
            A = {(a, b): float(sum(w * (J[a] * J[b]))) for a in range(3) for b in range(a, 3)}
            g = [float(sum(w * (J[a] * r))) for a in range(3)]
            sw, swrr = float(sum(w)), float(sum(w * (r * r)))
            used, count = it + 1, int(k.sum())
            rms = np.sqrt(np.float64(swrr) / np.float64(sw))
            if count < 3:
                failed, obs = True, 0.0
                break
            dmax = max(A[0, 0], max(A[1, 1], A[2, 2]))
            floor_ = min_pivot * dmax
            pivots = [A[0, 0]]
            failed = not pivots[0] > floor_
            if not failed:
                l00 = np.sqrt(pivots[0])
                l10, l20 = A[0, 1] / l00, A[0, 2] / l00
                pivots.append(A[1, 1] - l10 * l10)
                failed = not pivots[1] > floor_
                if not failed:
                    l11 = np.sqrt(pivots[1])
                    l21 = (A[1, 2] - l20 * l10) / l11
                    pivots.append((A[2, 2] - l20 * l20) - l21 * l21)
                    failed = not pivots[2] > floor_
                    if not failed:
                        l22 = np.sqrt(pivots[2])
            obs = min(pivots) / dmax if dmax > 0.0 else 0.0
            if dmax > 0.0:
                margins.take("pivot", [abs(p / dmax - min_pivot) for p in pivots])
            if failed:
                break
            y0 = -g[0] / l00
            y1 = (-g[1] - l10 * y0) / l11
            y2 = ((-g[2] - l20 * y0) - l21 * y1) / l22
            x2 = y2 / l22
            x1 = (y1 - l21 * x2) / l11
            x0 = ((y0 - l10 * x1) - l20 * x2) / l00
            c0, s0 = np.cos(x0), np.sin(x0)
            th, ux, uy = th + x0, (c0 * ux - s0 * uy) + x1, (s0 * ux + c0 * uy) + x2
            margins.take("stop", [abs(abs(x0) - eps_theta), abs(max(abs(x1), abs(x2)) - eps_u)])
            if abs(x0) < eps_theta and max(abs(x1), abs(x2)) < eps_u:
                break
        corr, res = np.full(N, -1, np.int32), np.full((N, 2), np.nan)
        if not failed:
            k, j, _, (dx, dy), _ = _correspond(ax, ay, px, py, valid, th, ux, uy, centres, window, gate2, gap2, margins)
            c, s = np.cos(th), np.sin(th)
            corr[k] = j[k]
            res[k] = np.stack([c * dx + s * dy, (-s) * dx + c * dy], axis=1)[k]
    return failed, np.array([th, ux, uy]), count, rms, used, obs, corr, res


def match_oracle(r_prev, r_cur, tab, init=None, person=None, max_range=20.0, window=16, gate=0.5, max_gap=0.3,
                 huber_delta=0.05, iters=16, eps_theta=1e-7, eps_u=1e-7, min_pivot=1e-6, sum=np.sum):
    """The formulas of pof_scan_match for one scan pair in float64.  r_prev, r_cur [N] float32, tab [3N] the angle
    table, init [3] or None, person [N] bool: current points that do not vote (``person_points``).  `sum` adds a 1-D
    array (np.sum: pairwise; seq_sum).  -> dict motion [3], ok, count, rms, iters_used, obs, corr [N], flow_residual
    [N,2], and margins: the smallest margin of every kind of discrete decision taken, and their number."""
    r0, r1 = np.asarray(r_prev, np.float32), np.asarray(r_cur, np.float32)
    N = len(r0)
    tab = np.asarray(tab, np.float64)
    cs, sn = tab[N::2], tab[N + 1::2]
    dphi = tab[1] - tab[0] if N > 1 else 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        v0 = np.isfinite(r0) & (r0.astype(np.float64) < max_range)
        valid = np.isfinite(r1) & (r1.astype(np.float64) < max_range)
        ax, ay = np.where(v0, r0.astype(np.float64) * cs, np.nan), np.where(v0, r0.astype(np.float64) * sn, np.nan)
        px, py = r1.astype(np.float64) * cs, r1.astype(np.float64) * sn
    if person is not None:
        valid = valid & ~np.asarray(person, bool)
    if init is None or not np.isfinite(np.asarray(init, np.float64)).all():
        init = np.zeros(3)
    margins = _Margins()
    failed, motion, count, rms, used, obs, corr, res = _iterate(ax, ay, px, py, valid, init, _shift_centres(dphi, N),
                                                                window, gate, max_gap, huber_delta, iters, eps_theta,
                                                                eps_u, min_pivot, sum, margins)
    nan = np.nan
    return {"motion": np.full(3, nan) if failed else motion, "ok": np.uint8(not failed),
            "count": np.int32(count), "rms": nan if failed else float(rms), "iters_used": np.int32(used),
            "obs": float(obs), "corr": corr, "flow_residual": res, "margins": margins}


FLOATS, EXACT = ("motion", "rms", "obs", "flow_residual"), ("count", "ok", "iters_used", "corr")


def tolerance(cases):
    """TOL for device-against-oracle over `cases` = [(args, kwargs) of match_oracle]: 100 x the largest disagreement of
    the pairwise and the sequential evaluation, at least 1e-13, never above 1e-10; every decision margin of the cases
    is asserted to be >= MARGIN_MIN.  -> (tol, the pairwise results)."""
    worst, results, smallest, decisions = 0.0, [], {}, 0
    for args, kw in cases:
        a, b = match_oracle(*args, **kw), match_oracle(*args, sum=seq_sum, **kw)
        for key in EXACT:
            assert np.array_equal(a[key], b[key]), key
        for key in FLOATS:
            x, y = np.asarray(a[key], np.float64), np.asarray(b[key], np.float64)
            assert np.array_equal(np.isfinite(x), np.isfinite(y)), key
            both = np.isfinite(x)
            worst = max(worst, np.abs(x[both] - y[both]).max(initial=0.0))
        for kind, v in a["margins"].items():
            if kind == "decisions":
                decisions += v
            else:
                smallest[kind] = min(smallest.get(kind, np.inf), v)
        results.append(a)
    tol = max(1e-13, 100.0 * worst)
    print("pairwise against sequential: %.3e -> TOL %.3e; %d decisions, smallest margins %s"
          % (worst, tol, decisions, {k: "%.2e" % v for k, v in sorted(smallest.items())}))
    assert tol <= 1e-10
    assert all(v >= MARGIN_MIN for v in smallest.values()), smallest
    return tol, results


def assert_matches(got, want, tol, what=""):
    """Device outputs of one pair (dict of arrays) against the oracle's: count / ok / iters_used / corr exact, the rest
    within tol, NaN where the oracle has NaN."""
    for key in EXACT:
        assert np.array_equal(np.asarray(got[key]), np.asarray(want[key])), (what, key, got[key], want[key])
    for key in FLOATS:
        x, y = np.asarray(got[key], np.float64), np.asarray(want[key], np.float64)
        assert np.array_equal(np.isnan(x), np.isnan(y)), (what, key)
        fin = np.isfinite(y)
        assert np.array_equal(x[~fin], y[~fin], equal_nan=True), (what, key)
        err = np.abs(x[fin] - y[fin]).max(initial=0.0)
        assert err <= tol, (what, key, err, tol)


# ---------------------------------------------------------------- tests (no GPU)
TAB = angle_table(450)


def _recover(pairs, bound, max_iters, what, **kw):
    worst, most = 0.0, 0
    for n, (r0, r1, true, step) in enumerate(pairs):
        res = match_oracle(r0, r1, TAB, **kw)
        err = motion_error(res["motion"], true)
        print("%s %d: step %.3e m, error %.3e m, %d iterations, %d matched, rms %.2e, obs %.2e"
              % (what, n, step, err, res["iters_used"], res["count"], res["rms"], res["obs"]))
        assert res["ok"] and err <= bound and err <= 0.1 * step and res["iters_used"] <= max_iters
        worst, most = max(worst, err), max(most, int(res["iters_used"]))
    print("%s: worst error %.3e m (bound %.3e), at most %d iterations" % (what, worst, bound, most))
    return worst


def test_recovers_the_odometry_step_on_clean_rooms():
    _recover(room_pairs(8), BOUND_CLEAN, ITERS_CLEAN, "clean")


def test_recovers_the_step_under_range_noise():
    _recover(room_pairs(8, noise=0.01), BOUND_NOISE, ITERS_NOISE, "1 cm noise")


def test_recovers_a_four_times_larger_step_under_range_noise():
    _recover(room_pairs(8, noise=0.01, scale=4.0), BOUND_NOISE_BIG, ITERS_NOISE_BIG, "1 cm noise, 4 x step")


def test_the_true_motion_as_init_converges_at_once():
    for n, (r0, r1, true, _) in enumerate(room_pairs(8)):
        res = match_oracle(r0, r1, TAB, init=true)
        print("init = truth %d: %d iterations, error %.3e" % (n, res["iters_used"], motion_error(res["motion"], true)))
        assert res["ok"] and res["iters_used"] <= 2 and motion_error(res["motion"], true) <= BOUND_CLEAN
        # a row that is not finite counts as zeros
        rest = match_oracle(r0, r1, TAB)
        bad = match_oracle(r0, r1, TAB, init=[np.nan, 0.1, 0.1])
        assert np.array_equal(bad["motion"], rest["motion"]) and bad["iters_used"] == rest["iters_used"]


def test_gated_people_do_not_disturb_the_fit():
    rng = np.random.default_rng(77)
    for n, (r0, r1, true, step) in enumerate(room_pairs(8)):
        r1p, inst, num, det_cls = add_people(r1, rng)
        person = person_points(inst, num, det_cls)
        assert 0.19 * len(r1) <= person.sum() <= 0.2 * len(r1) and (inst[~person] > 0).any()
        gated = match_oracle(r0, r1p, TAB, person=person)
        err = motion_error(gated["motion"], true)
        print("people %d: gated error %.3e m, %d matched" % (n, err, gated["count"]))
        assert gated["ok"] and err <= BOUND_CLEAN and err <= 0.1 * step
        assert gated["count"] <= len(r1) - person.sum() and (gated["corr"][person] == -1).all()
        assert np.isnan(gated["flow_residual"][person]).all()


def corridor(N=450, half_width=1.5):
    """Two parallel walls either side of the sensor, open ends (beyond max_range), seen from two poses along it."""
    phi = R.laser_phi(num_pts=N)
    segs = np.array([[(-200.0, half_width), (200.0, half_width)], [(-200.0, -half_width), (200.0, -half_width)]])
    cast = lambda pose: np.minimum(ray_cast(segs, pose, phi), 29.99).astype(np.float32)
    return cast(np.array([0.0, 0.0, 0.0])), cast(np.array([0.04, 0.0, 0.0]))


def test_failures_are_reported():
    r0, r1, _, _ = room_pairs(1)[0]
    far = np.full(450, 29.99, np.float32)
    for prev, cur in ((far, r1), (r0, far), (far, far)):       # all ranges >= max_range
        res = match_oracle(prev, cur, TAB)
        assert not res["ok"] and np.isnan(res["motion"]).all() and np.isnan(res["rms"]) and res["count"] == 0
        assert res["iters_used"] == 1 and res["obs"] == 0.0 and (res["corr"] == -1).all()
        assert np.isnan(res["flow_residual"]).all()
    two = far.copy()
    two[100:102] = r1[100:102]                                 # fewer than 3 matches
    res = match_oracle(r0, two, TAB)
    assert not res["ok"] and res["count"] == 2 and np.isnan(res["motion"]).all() and res["obs"] == 0.0
    c0, c1 = corridor()
    res = match_oracle(c0, c1, TAB)
    print("corridor: obs %.3e, %d matched" % (res["obs"], res["count"]))
    assert not res["ok"] and res["count"] > 100 and res["obs"] <= 1e-6 and np.isnan(res["motion"]).all()
    assert match_oracle(r0, r1, TAB)["obs"] > 1e-3             # a room is well observed


def test_summation_order_the_tolerance_rule_and_the_decision_margins():
    """Every committed case of the GPU tests' 450-point shapes keeps its decision margins."""
    cases = [((r0, r1, TAB), {}) for r0, r1, _, _ in room_pairs(8)]
    cases += [((r0, r1, TAB), {}) for r0, r1, _, _ in room_pairs(8, noise=0.01)]
    cases += [((r0, r1, TAB), dict(huber_delta=0.0)) for r0, r1, _, _ in room_pairs(4, noise=0.01, scale=4.0)]
    tolerance(cases)


def test_abi_and_python_surface():
    import ctypes
    import os
    from planar_optical_flow_amd import _lib, build, ops
    build.build(verbose=False)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pof_abi.h")).read()
    assert "pof_scan_match" in _lib.SIGNATURES and "int pof_scan_match(" in header
    assert "N8 scan-to-scan matching" in header and "utils.py:639-662" in header
    assert len(_lib.SIGNATURES["pof_scan_match"][1]) == 28
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "pof_scan_match") and hasattr(_lib.load(), "pof_scan_match")
    assert ops.ScanMatch._fields == ("motion", "count", "rms", "ok", "iters_used", "obs", "corr", "flow_residual")
    assert callable(ops.scan_match_buffers)
    # the library's own argument checks, before any launch: no pointer is dereferenced
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    args = lambda **kw: [one, one, one, None, None, None, None, 0.5, 20.0, kw.get("window", 16), kw.get("gate", 0.5),
                         kw.get("max_gap", 0.3), kw.get("huber_delta", 0.05), kw.get("iters", 16), 1e-7, 1e-7, 1e-6,
                         kw.get("B", 1), kw.get("N", 450), one, one, one, one, one, one, None, None, None]
    for bad in (dict(window=0), dict(window=65), dict(iters=0), dict(iters=33), dict(gate=-1.0), dict(max_gap=-0.1),
                dict(huber_delta=-0.05), dict(gate=float("nan")), dict(B=-1), dict(N=0)):
        assert lib.pof_scan_match(*args(**bad)) == _lib.POF_E_BADARG, bad
    assert lib.pof_scan_match(*args(N=4097)) == _lib.POF_E_SHAPE
    assert lib.pof_scan_match(*args(B=0)) == _lib.POF_OK


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    import torch
    from planar_optical_flow_amd import ops
    B, N = 2, 8
    prev, cur, tab = torch.ones(B, N), torch.ones(B, N), torch.zeros(3 * N, dtype=torch.float64)
    with pytest.raises(TypeError):
        ops.scan_match(prev, cur, tab)
    for bad in (dict(window=0), dict(window=65), dict(iters=0), dict(iters=33), dict(gate=-0.5), dict(max_gap=-0.3),
                dict(huber_delta=-1.0), dict(gate=float("nan")),
                dict(instance_mask=torch.zeros(B, N, dtype=torch.int32), num_det=torch.zeros(B, dtype=torch.int32))):
        with pytest.raises(ValueError):
            ops.scan_match(prev, cur, tab, **bad)
    sig = inspect.signature(ops.scan_match)
    assert list(sig.parameters) == ["ranges_prev", "ranges_cur", "tab", "init", "instance_mask", "num_det", "det_cls",
                                    "cls_thresh", "max_range", "window", "gate", "max_gap", "huber_delta", "iters",
                                    "eps_theta", "eps_u", "min_pivot", "out"]
    assert {k: sig.parameters[k].default for k in DEFAULTS} == DEFAULTS
    assert all(p.kind is p.KEYWORD_ONLY for p in list(sig.parameters.values())[3:])


def test_utils_and_streaming_signatures():
    from planar_optical_flow_amd.src.utils import utils as u
    from planar_optical_flow_amd.streaming import StreamingDetector
    sig = inspect.signature(u.scan_match)
    assert list(sig.parameters) == ["scan_prev", "scan_cur", "scan_phi", "pred_cls", "pred_reg", "kw"]
    assert sig.parameters["kw"].kind is inspect.Parameter.VAR_KEYWORD
    assert inspect.signature(StreamingDetector.__init__).parameters["ego_motion"].default is None
    src = inspect.getsource(StreamingDetector)
    assert "scan_match" in src and "_match_out" in src
