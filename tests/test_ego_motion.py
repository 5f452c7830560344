"""Ego-motion from a flow field (pof_ego_motion / pof_pose_advance, N6) without a GPU: a NumPy restatement of the
device's formulas (``ego_oracle``), pinned to the reference through tests/golden/scan_geometry.npz -- the fit is the
exact inverse of get_displacement_from_odometry (src/utils/utils.py:639-662) and get_velocity_from_odometry
(:609-636), whose outputs that fixture holds -- and the host-side argument checks.  tests/test_ego_motion_gpu.py
imports the helpers below.

Bounds against the odometry (``ODOM_TOL``): the reference stores its rotation matrices in float32, 2^-24 per entry, two
entries per component, acting on points of ~8 m mean range: 1e-6 rad / m for the rigid fit of the displacement.  The
velocity's float32 matrices act on |dt| <= 0.07 m only: 1e-8.
Device against oracle (``tolerance``): the two differ in the order of their sums and in the last bit of hypot / atan2 /
sincos, so the tolerance is 100 x the largest disagreement between the oracle's own pairwise and sequential
evaluations on the inputs at hand, at least 1e-13 (the libm share) and asserted to stay below 1e-10."""
import inspect

import numpy as np
import pytest

from oracle import ref_numpy as R
from planar_optical_flow_amd import synth

ODOM_TOL_RIGID = 1e-6
ODOM_TOL_LINEAR = 1e-8


# ---------------------------------------------------------------- restatement of the device arithmetic, one scan
def seq_sum(x):
    """Plain IEEE double adds in index order."""
    total = 0.0
    for v in np.asarray(x, dtype=np.float64).tolist():
        total += v
    return total


def base_weights(p, f, weight=None, ranges=None, max_range=20.0, inst=None, num=None, det_cls=None, cls_thresh=0.5):
    """w0 [N] of one scan: the weight (or 1), zero where it is not finite or <= 0, where the range is not finite or
    >= max_range, where a flow or point component is not finite, and on the points of detections with
    det_cls >= cls_thresh (ids 1..clamp(num, 0, N))."""
    n = len(p)
    w = np.ones(n) if weight is None else np.asarray(weight, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        w = np.where(np.isfinite(w) & (w > 0), w, 0.0)
        if ranges is not None:
            r = np.asarray(ranges, np.float32)
            w = np.where(np.isfinite(r) & (r.astype(np.float64) < max_range), w, 0.0)
    w = np.where(np.isfinite(f).all(axis=1) & np.isfinite(p).all(axis=1), w, 0.0)
    if inst is not None:
        nd = min(max(int(num), 0), n)
        ids = np.asarray(inst, np.int64)
        member = (ids >= 1) & (ids <= nd)
        person = np.zeros(n, bool)
        person[member] = np.asarray(det_cls)[ids[member] - 1] >= cls_thresh
        w = np.where(person, 0.0, w)
    return w


def _residual(model, m, p, h):
    if model == 0:
        th, ux, uy = m
        c, s = np.cos(th), np.sin(th)
        return np.stack([(c * p[:, 0] - s * p[:, 1]) + ux - h[:, 0], (s * p[:, 0] + c * p[:, 1]) + uy - h[:, 1]], axis=1)
    om, tx, ty = m
    return np.stack([(tx + om * (-p[:, 1])) - h[:, 0], (ty + om * p[:, 0]) - h[:, 1]], axis=1)


def ego_oracle(p, f, w0, sign, model, huber_delta=0.0, iters=0, sum=np.sum):
    """The formulas of pof_ego_motion for one scan in float64: p [N,2] points, f [N,2] scanner-frame flow, w0 [N]
    base weights (``base_weights``), model 0 rigid / 1 linear.  `sum` adds a 1-D array (np.sum: pairwise; seq_sum).
    -> dict motion [3], ok, count, rms, flow_residual [N,2], weight [N] float32."""
    p, f, w0 = np.asarray(p, np.float64), np.asarray(f, np.float64), np.asarray(w0, np.float64)
    g = float(sign) * f
    h = p + g if model == 0 else g
    w = w0.copy()
    n_it = int(iters) if huber_delta > 0 else 0
    nan3 = np.full(3, np.nan)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for it in range(n_it + 1):
            k = w > 0
            wk, pk, hk = w[k], p[k], h[k]
            W = sum(wk)
            pm = np.array([sum(wk * pk[:, 0]) / W, sum(wk * pk[:, 1]) / W]) if k.any() else np.full(2, np.nan)
            hm = np.array([sum(wk * hk[:, 0]) / W, sum(wk * hk[:, 1]) / W]) if k.any() else np.full(2, np.nan)
            d, e = pk - pm, hk - hm
            s_pp = sum(wk * (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]))
            s_dot = sum(wk * (d[:, 0] * e[:, 0] + d[:, 1] * e[:, 1]))
            s_x = sum(wk * (d[:, 0] * e[:, 1] - d[:, 1] * e[:, 0]))
            failed = int(k.sum()) < 2 or not s_pp > 0
            if failed:
                m = nan3
            elif model == 0:
                th = np.arctan2(s_x, s_dot)
                c, s = np.cos(th), np.sin(th)
                m = np.array([th, hm[0] - (c * pm[0] - s * pm[1]), hm[1] - (s * pm[0] + c * pm[1])])
            else:
                om = s_x / s_pp
                m = np.array([om, hm[0] - om * (-pm[1]), hm[1] - om * pm[0]])
            if failed or it == n_it:
                break
            rho = np.hypot(*_residual(model, m, p, h).T)
            w = w0 * np.where(rho > huber_delta, huber_delta / rho, 1.0)
        e = _residual(model, m, p, h)
        rho = np.hypot(e[:, 0], e[:, 1])
        k = w > 0
        rms = np.nan if failed else np.sqrt(sum(w[k] * (rho[k] * rho[k])) / W)
    return {"motion": m, "ok": np.uint8(not failed), "count": np.int32((w0 > 0).sum()), "rms": rms,
            "flow_residual": -float(sign) * e, "weight": w.astype(np.float32)}


def tolerance(cases):
    """TOL for device-against-oracle over `cases` = [(args, kwargs) of ego_oracle]: 100 x the largest disagreement of
    the pairwise and the sequential evaluation, at least 1e-13; and the pairwise results.  Never above 1e-10."""
    worst, results = 0.0, []
    for args, kw in cases:
        a, b = ego_oracle(*args, **kw), ego_oracle(*args, sum=seq_sum, **kw)
        for key in ("motion", "rms", "flow_residual"):
            x, y = np.asarray(a[key], np.float64), np.asarray(b[key], np.float64)
            both = np.isfinite(x) & np.isfinite(y)
            assert np.array_equal(np.isfinite(x), np.isfinite(y))
            worst = max(worst, np.abs(x[both] - y[both]).max(initial=0.0))
        results.append(a)
    tol = max(1e-13, 100.0 * worst)
    print("pairwise against sequential: %.3e -> TOL %.3e" % (worst, tol))
    assert tol <= 1e-10
    return tol, results


def assert_matches(got, want, tol, what=""):
    """Device outputs of one scan (dict of arrays) against the oracle's: count / ok exact, the rest within tol, NaN
    where the oracle has NaN."""
    assert int(got["count"]) == int(want["count"]) and int(got["ok"]) == int(want["ok"]), (what, got["count"], want["count"])
    for key in ("motion", "rms", "flow_residual"):
        x, y = np.asarray(got[key], np.float64), np.asarray(want[key], np.float64)
        assert np.array_equal(np.isnan(x), np.isnan(y)), (what, key)
        fin = np.isfinite(y)
        assert np.array_equal(x[~fin], y[~fin], equal_nan=True), (what, key)
        err = np.abs(x[fin] - y[fin]).max(initial=0.0)
        assert err <= tol, (what, key, err, tol)


def true_motion(odom0, odom1):
    """(theta, u) of the displacement convention and (omega, t) of the velocity, in float64, from a pose pair."""
    d = np.asarray(odom1, np.float64) - np.asarray(odom0, np.float64)
    rt = lambda a: np.array([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]])     # R(a)^T
    return (np.concatenate([[d[2]], rt(odom0[2]) @ d[:2]]), np.concatenate([[-d[2]], -(rt(odom1[2]) @ d[:2])]))


def rigid_field(p, theta, u):
    """The displacement p - (R(theta) p + u) of points p [N,2] in float64 (no float32 matrices: exactly rigid)."""
    c, s = np.cos(theta), np.sin(theta)
    return p - (np.stack([c * p[:, 0] - s * p[:, 1], s * p[:, 0] + c * p[:, 1]], axis=1) + np.asarray(u))


def motion_error(m, true):
    """max(8 |d theta|, |d u|_inf): an angle error acts on points of ~8 m range."""
    return max(8.0 * abs(m[0] - true[0]), np.abs(np.asarray(m[1:]) - true[1:]).max())


def robust_cases(n_scans, seed=11, N=450, outliers=90):
    """Seeded scans with ranges as SURVEY 8(d) and the synthetic odometry step; the displacement of a rigid scene with
    `outliers` of the N points given a person-like extra motion of 0.1-0.3 m in a random direction, rounded to
    float32.  -> list of (xy [N,2], disp float32 [N,2], true (theta, u))."""
    rng = np.random.default_rng(seed)
    phi = R.laser_phi(num_pts=N)
    out = []
    for _ in range(n_scans):
        a, c = rng.uniform(0, 2 * np.pi, 2)
        r = (np.clip(6 + 3 * np.sin(2 * phi + a) + 1.5 * np.sin(7 * phi + c), 0.3, 25) + rng.normal(0, 0.01, N)).astype(np.float32)
        xy = np.stack(R.polar_to_xy(r, phi), axis=1)
        odom0 = np.concatenate([rng.uniform(-5, 5, 2), rng.uniform(-np.pi, np.pi, 1)])
        odom1 = odom0 + np.concatenate([rng.uniform(-0.05, 0.05, 2), rng.uniform(-0.03, 0.03, 1)])
        disp = R.displacement_from_odometry(xy, odom0, odom1)
        idx = rng.choice(N, outliers, replace=False)
        mag, ang = rng.uniform(0.1, 0.3, outliers), rng.uniform(0, 2 * np.pi, outliers)
        disp[idx] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=1)
        out.append((xy, disp.astype(np.float32), true_motion(odom0, odom1)[0]))
    return out


def fixture_odometry():
    """The pose pairs tests/golden/scan_geometry.npz was generated with (tools/gen_golden.py)."""
    sb = synth.make_batch(seed=1, B=6, T=2, mixed_classes=True)
    return sb.odom0, sb.odom1


# ---------------------------------------------------------------- tests (no GPU)
def test_oracle_inverts_the_references_flow_targets(golden):
    g = golden("scan_geometry")
    odom0, odom1 = fixture_odometry()
    ones = np.ones(450)
    for b in range(6):
        rigid_true, linear_true = true_motion(odom0[b], odom1[b])
        for sum_ in (np.sum, seq_sum):
            rigid = ego_oracle(g["xy"][b], g["disp"][b], ones, -1, 0, sum=sum_)
            linear = ego_oracle(g["xy"][b], g["velocity"][b], ones, 1, 1, sum=sum_)
            er, el = np.abs(rigid["motion"] - rigid_true), np.abs(linear["motion"] - linear_true)
            print("scan %d: rigid %.2e rad %.2e m, linear %.2e" % (b, er[0], er[1:].max(), el.max()))
            assert rigid["ok"] and linear["ok"] and rigid["count"] == 450
            assert er.max() <= ODOM_TOL_RIGID and el.max() <= ODOM_TOL_LINEAR
            # the fitted motion explains the whole field: nothing is left over
            assert np.abs(rigid["flow_residual"]).max() <= 2e-5 and rigid["rms"] <= 2e-5


def test_summation_order_and_the_tolerance_rule(golden):
    g = golden("scan_geometry")
    ones = np.ones(450)
    plain = [((g["xy"][b], g["disp"][b], ones, -1, 0), {}) for b in range(6)]
    tol, _ = tolerance(plain)
    assert tol <= 1e-12                                        # the order of the sums stays near the libm share
    tolerance([((xy, d.astype(np.float64), ones, -1, 0), dict(huber_delta=0.02, iters=4)) for xy, d, _ in robust_cases(4)])


def test_huber_passes_halve_the_error_on_every_robust_scan():
    """The condition the GPU test holds the device to, on the oracle alone and on more scans."""
    ones = np.ones(450)
    ratios = []
    for xy, disp, true in robust_cases(40):
        d = disp.astype(np.float64)
        plain = motion_error(ego_oracle(xy, d, ones, -1, 0)["motion"], true)
        robust = motion_error(ego_oracle(xy, d, ones, -1, 0, huber_delta=0.02, iters=4)["motion"], true)
        ratios.append(plain / robust)
    print("plain / robust error: min %.2f median %.2f" % (min(ratios), np.median(ratios)))
    assert min(ratios) >= 2.0


def test_oracle_failures_and_gates():
    rng = np.random.default_rng(3)
    p, f = rng.normal(0, 5, (6, 2)), rng.normal(0, 0.05, (6, 2))
    for w0 in (np.zeros(6), np.eye(6)[0]):                    # nothing / one point
        res = ego_oracle(p, f, w0, -1, 0)
        assert not res["ok"] and np.isnan(res["motion"]).all() and np.isnan(res["rms"]) and res["count"] == w0.sum()
    assert not ego_oracle(np.ones((6, 2)), f, np.ones(6), -1, 0)["ok"]           # all at one place
    two = ego_oracle(p[:2], rigid_field(p[:2], 0.02, (0.04, -0.03)), np.ones(2), -1, 0)
    assert two["ok"] and two["rms"] <= 1e-12                   # two distinct points of a rigid field: an exact fit
    f[2, 0] = np.nan
    w = base_weights(p, f, weight=[1, -1, 1, np.nan, 0, 2], ranges=[1, 1, 1, 1, 1, 29.99],
                     inst=[0, 0, 0, 0, 1, 3], num=2, det_cls=[0.9, 0.1, 0.9, 0, 0, 0])
    assert np.array_equal(w, [1, 0, 0, 0, 0, 0])
    assert np.array_equal(base_weights(p, f, inst=[1, 2, 0, 3, 1, 2], num=2, det_cls=[0.9, 0.1, 0.9, 0, 0, 0]),
                          [0, 1, 0, 1, 0, 1])


def test_abi_and_python_surface():
    import os
    from planar_optical_flow_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pof_abi.h")).read()
    for name in ("pof_ego_motion", "pof_pose_advance"):
        assert name in _lib.SIGNATURES and ("int %s(" % name) in header
    assert "utils.py:639-662" in header and ":609-636" in header
    assert len(_lib.SIGNATURES["pof_ego_motion"][1]) == 25 and len(_lib.SIGNATURES["pof_pose_advance"][1]) == 8


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    import torch
    from planar_optical_flow_amd import ops
    B, N = 2, 8
    ranges, tab, flow = torch.ones(B, N), torch.zeros(3 * N, dtype=torch.float64), torch.zeros(B, N, 2)
    with pytest.raises(TypeError):
        ops.ego_motion(ranges, tab, flow)
    with pytest.raises(TypeError):
        ops.pose_advance(torch.zeros(B, 3, dtype=torch.float64), torch.ones(B, dtype=torch.uint8),
                         torch.zeros(B, 3, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.ego_motion(ranges, tab, flow, sign=0)
    with pytest.raises(ValueError):
        ops.ego_motion(ranges, tab, flow, iters=17)
    with pytest.raises(ValueError):
        ops.ego_motion(ranges, tab, flow, model="affine")
    with pytest.raises(ValueError):
        ops.ego_motion(ranges, tab, flow, instance_mask=torch.zeros(B, N, dtype=torch.int32),
                       num_det=torch.zeros(B, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.ego_motion(None, tab, flow)
    assert ops.EgoMotion._fields == ("motion", "count", "rms", "ok", "flow_residual", "weight")
    assert callable(ops.ego_motion_buffers)


def test_utils_names_and_signatures():
    from planar_optical_flow_amd.src.utils import utils as u
    names = lambda fn: list(inspect.signature(fn).parameters)
    assert names(u.get_odometry_from_displacement) == ["scan1_xy", "disp", "odom0", "weight", "huber_delta", "iters"]
    assert names(u.get_odometry_from_velocity) == ["scan1_xy", "v_dt", "odom0", "weight", "huber_delta", "iters"]
    sig = inspect.signature(u.ego_motion)
    assert list(sig.parameters) == ["scan", "scan_phi", "pred_flow", "pred_cls", "pred_reg", "min_dist", "cls_thresh",
                                    "max_range", "huber_delta", "iters"]
    assert [sig.parameters[k].default for k in ("min_dist", "cls_thresh", "max_range", "huber_delta", "iters")] == \
        [0.5, 0.5, 20.0, 0.02, 4]
    from planar_optical_flow_amd.streaming import StreamingDetector
    assert inspect.signature(StreamingDetector.__init__).parameters["ego_motion"].default is None
    assert "pose" in inspect.signature(StreamingDetector.reset).parameters
