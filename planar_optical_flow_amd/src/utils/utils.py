"""Drop-in for the reference's ``src/utils/utils.py`` scan-geometry functions.

Same names, argument order and defaults as the reference (citations are
``src/utils/utils.py:line`` of the reference checkout).  Every function runs on
the MI355X through libpof_hip.so:

* NumPy arguments are copied to the device, processed by the HIP kernel and the
  result is returned as NumPy with the reference's dtype (a convenience path
  for code that still calls per scan -- one launch per call, latency bound);
* torch device tensors are processed in place of residence and tensors are
  returned.  Batched inputs ([B,N] ranges, [B,T,N] windows) are accepted
  wherever the arithmetic is per point -- that is the fast path, see
  ``planar_optical_flow_amd.ops``.

There is no CPU fallback: without a HIP device these functions raise.
"""
import numpy as np
import torch

from planar_optical_flow_amd import ops

_DEFAULT_INC = np.radians(0.5)


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("planar_optical_flow_amd needs a HIP device (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _is_t(x):
    return isinstance(x, torch.Tensor)


def _to_dev(x, dtype):
    if _is_t(x):
        return x.to(device=_device(), dtype=dtype).contiguous()
    arr = np.ascontiguousarray(x, dtype={torch.float32: np.float32, torch.float64: np.float64,
                                         torch.int32: np.int32}[dtype])
    if not arr.flags.writeable:
        arr = arr.copy()
    return torch.from_numpy(arr).to(_device())


def _host(t):
    """Row 0 of a device tensor -- the one scan of a per-scan call -- as NumPy."""
    return t[0].cpu().numpy()


def _nms(ranges, tab, pred_cls, pred_reg, min_dist):
    """The centre NMS of one scan from host-side predictions: ranges [1,N] on the device, pred_cls [N,1] (scores),
    pred_reg [N,2] -> (det_xy, det_cls, num_det, instance_mask) as ``ops.nms_predicted_center`` returns them, and the
    dtype of the scores, which the reference's det_cls keeps."""
    pc = pred_cls.detach().cpu().numpy() if _is_t(pred_cls) else np.asarray(pred_cls)
    assert pc.ndim == 2 and pc.shape[1] == 1
    return (*ops.nms_predicted_center(ranges, tab, _to_dev(pc[:, 0], torch.float64).reshape(1, -1),
                                      _to_dev(pred_reg, torch.float64).reshape(1, -1, 2), min_dist), pc.dtype)


def _stage_kw(wrapper, name, kw, *elsewhere):
    """kw, the settings a class passes on to the ``ops`` wrapper of its stage: a key that is not one of the wrapper's
    settings (``ops.stage_settings``; ``elsewhere``: those the class takes by another way) raises."""
    unknown = set(kw) - (set(ops.stage_settings(wrapper)) - set(elsewhere))
    if unknown:
        raise ValueError("unknown %s settings: %s" % (name, sorted(unknown)))
    return kw


def _grid_of(scan_phi):
    """(angle_inc, N) of a uniformly spaced angle grid given as array/tensor."""
    phi = scan_phi.detach().cpu().numpy() if _is_t(scan_phi) else np.asarray(scan_phi)
    n = phi.shape[-1]
    assert n >= 2, "angle grid needs at least two points"
    inc = float((phi[-1] - phi[0]) / (n - 1))
    return inc, n


def _table_for(scan_phi):
    """Device angle table matching `scan_phi`.  The kernels regenerate the grid
    from (angle_inc, N) exactly as get_laser_phi does; a grid that is not the
    linspace of its end points is rejected."""
    inc, n = _grid_of(scan_phi)
    tab = ops.phi_table(inc, n, _device())
    ref = tab[:n]
    got = _to_dev(scan_phi, torch.float64).reshape(-1)
    if not torch.allclose(ref, got, rtol=0, atol=1e-9):
        raise AssertionError("scan_phi must be a uniform angle grid (get_laser_phi)")
    return tab


# ------------------------------------------------------------------ A1
def get_laser_phi(angle_inc=np.radians(0.5), num_pts=450):
    """:25-29.  Evaluated on the device (bit-identical to numpy.linspace)."""
    return ops.laser_phi(angle_inc, num_pts, _device()).cpu().numpy()


# ------------------------------------------------------------------ A2
def rphi_to_xy(r, phi):
    """:47-48."""
    tensor_in = _is_t(r)
    rr = _to_dev(r, torch.float32 if (tensor_in and r.dtype == torch.float32) or
                 (not tensor_in and np.asarray(r).dtype == np.float32) else torch.float64)
    n = rr.shape[-1] if rr.dim() else 1
    phi_arr = phi.detach().cpu().numpy() if _is_t(phi) else np.asarray(phi, dtype=np.float64)
    if rr.dim() == 0 or phi_arr.ndim == 0 or rr.dtype != torch.float32 or phi_arr.shape[-1] != n or n < 2:
        # scalar / non-grid use (e.g. a single detection): r*cos, r*sin elementwise on the device
        p = _to_dev(phi_arr, torch.float64)
        x, y = rr.double() * torch.cos(p), rr.double() * torch.sin(p)
    else:
        tab = _table_for(phi_arr)
        flat = rr.reshape(-1, n)
        out = ops.scan_preprocess(flat, tab, out_dtype=torch.float64, want=("xy",))["xy"]
        x, y = out[..., 0].reshape(rr.shape), out[..., 1].reshape(rr.shape)
    if tensor_in:
        return x, y
    return x.cpu().numpy(), y.cpu().numpy()


def rphi_to_xy_torch(r, phi):
    """:51-52."""
    return rphi_to_xy(r, phi)


def scan_to_xy(scan, phi=None):
    """:32-36."""
    return rphi_to_xy(scan, get_laser_phi() if phi is None else phi)


def xy_to_rphi(x, y):
    """:39-43."""
    tensor_in = _is_t(x)
    r, p = ops.xy_to_rphi(_to_dev(x, torch.float64), _to_dev(y, torch.float64))
    return (r, p) if tensor_in else (r.cpu().numpy(), p.cpu().numpy())


# ------------------------------------------------------------------ A4
def _rotate(flow, scan_phi, to_canonical, force_f32=False):
    tensor_in = _is_t(flow)
    dt = torch.float32 if (force_f32 or (tensor_in and flow.dtype == torch.float32)) else torch.float64
    f = _to_dev(flow, dt)
    out = ops.rotate_flow(f, _table_for(scan_phi), to_canonical)
    return out if tensor_in else out.cpu().numpy()


def global_to_canonical_flow(flow, scan_phi):
    """:62-75."""
    return _rotate(flow, scan_phi, True)


def canonical_to_global_flow(flow_canonical, scan_phi):
    """:78-89."""
    return _rotate(flow_canonical, scan_phi, False)


def canonical_to_global_flow_torch(flow_canonical, scan_phi):
    """:92-105 (float32; the rotation table stays resident on the device instead
    of being rebuilt and copied every call)."""
    return _rotate(flow_canonical, scan_phi, False, force_f32=True)


# ------------------------------------------------------------------ A5
def global_to_canonical(scan_r, scan_phi, dets_r, dets_phi):
    """:55-59.  Per point: scan_r/scan_phi [N] (or [B,N]), dets_* broadcastable."""
    tensor_in = _is_t(scan_r)
    r = _to_dev(scan_r, torch.float32)
    r2 = r.reshape(-1, r.shape[-1])
    dr = _to_dev(np.broadcast_to(dets_r.cpu().numpy() if _is_t(dets_r) else dets_r, tuple(r.shape)), torch.float64)
    dp = _to_dev(np.broadcast_to(dets_phi.cpu().numpy() if _is_t(dets_phi) else dets_phi, tuple(r.shape)),
                 torch.float64)
    dx, dy = ops.det_to_canonical(r2, _table_for(scan_phi), dr.reshape(r2.shape), dp.reshape(r2.shape))
    dx, dy = dx.reshape(r.shape), dy.reshape(r.shape)
    return (dx, dy) if tensor_in else (dx.cpu().numpy(), dy.cpu().numpy())


def canonical_to_global(scan_r, scan_phi, dx, dy):
    """:109-116."""
    tensor_in = _is_t(scan_r)
    r = _to_dev(scan_r, torch.float32)
    r2 = r.reshape(-1, r.shape[-1])
    ddx = _to_dev(dx, torch.float64).reshape(r2.shape)
    ddy = _to_dev(dy, torch.float64).reshape(r2.shape)
    dr, dp = ops.canonical_to_det(r2, _table_for(scan_phi), ddx, ddy)
    dr, dp = dr.reshape(r.shape), dp.reshape(r.shape)
    return (dr, dp) if tensor_in else (dr.cpu().numpy(), dp.cpu().numpy())


def canonical_to_global_torch(scan_r, scan_phi, dx, dy):
    """:119-126."""
    return canonical_to_global(scan_r, scan_phi, dx, dy)


# ------------------------------------------------------------------ A3
def _flow(kind, r, scan_phi, odom0, odom1, canonical):
    tab = _table_for(scan_phi)
    rr = _to_dev(r, torch.float32).reshape(1, -1)
    o0 = _to_dev(np.asarray(odom0, dtype=np.float64).reshape(1, 3), torch.float64)
    o1 = _to_dev(np.asarray(odom1, dtype=np.float64).reshape(1, 3), torch.float64)
    out = ops.scan_preprocess(rr, tab, o0, o1, flow_kind=kind, canonical=canonical, out_dtype=torch.float64,
                              want=("flow",))
    return out["flow"][0].cpu().numpy()


def _flow_xy(kind, xy, odom0, odom1):
    tensor_in = _is_t(xy)
    p = _to_dev(xy, torch.float64).reshape(1, -1, 2)
    o0 = _to_dev(np.asarray(odom0, dtype=np.float64).reshape(1, 3), torch.float64)
    o1 = _to_dev(np.asarray(odom1, dtype=np.float64).reshape(1, 3), torch.float64)
    out = ops.flow_from_xy(p, o0, o1, kind)[0]
    return out if tensor_in else out.cpu().numpy()


def get_flow_target(scan, scan_phi, odom_0, odom_1, to_canonical=False):
    """:204-229."""
    return _flow(ops.FLOW_TARGET, scan, scan_phi, odom_0, odom_1, to_canonical)


def get_displacement_from_odometry(scan1_xy, odom0, odom1):
    """:639-662."""
    return _flow_xy(ops.FLOW_DISPLACEMENT, scan1_xy, odom0, odom1)


def get_velocity_from_odometry(scan1_xy, odom0, odom1):
    """:609-636."""
    return _flow_xy(ops.FLOW_VELOCITY, scan1_xy, odom0, odom1)


# ------------------------------------------------------------------ N6: the two functions above, inverted
def _fit_xy(scan1_xy, flow, sign, model, weight, huber_delta, iters):
    xy = _to_dev(scan1_xy, torch.float64).reshape(1, -1, 2)
    res = ops.ego_motion(None, None, _to_dev(flow, torch.float64).reshape(1, -1, 2), xy=xy, canonical=False, sign=sign,
                         model=model, weight=None if weight is None else _to_dev(weight, torch.float32).reshape(1, -1),
                         huber_delta=huber_delta, iters=iters)
    return res.motion[0].cpu().numpy()


def get_odometry_from_displacement(scan1_xy, disp, odom0, weight=None, huber_delta=0.0, iters=0):
    """Inverse of ``get_displacement_from_odometry`` (:639-662): the rigid least-squares fit of scan1_xy ->
    scan1_xy - disp, composed onto odom0 = (x, y, phi).  -> odom1 [3] (NaN where the fit fails: fewer than two points,
    or all at one place).  weight [N], huber_delta, iters: as ``ops.ego_motion``."""
    th, ux, uy = _fit_xy(scan1_xy, disp, -1, "rigid", weight, huber_delta, iters)
    odom0 = np.asarray(odom0, dtype=np.float64)
    c, s = np.cos(odom0[2]), np.sin(odom0[2])
    return np.array([odom0[0] + (c * ux - s * uy), odom0[1] + (s * ux + c * uy), odom0[2] + th])


def get_odometry_from_velocity(scan1_xy, v_dt, odom0, weight=None, huber_delta=0.0, iters=0):
    """Inverse of ``get_velocity_from_odometry`` (:609-636): the linear fit v_dt = t + omega * (-y, x); the heading
    changes by -omega and the position by -R(phi1) t.  -> odom1 [3]."""
    om, tx, ty = _fit_xy(scan1_xy, v_dt, 1, "linear", weight, huber_delta, iters)
    odom0 = np.asarray(odom0, dtype=np.float64)
    phi1 = odom0[2] - om
    c, s = np.cos(phi1), np.sin(phi1)
    return np.array([odom0[0] - (c * tx - s * ty), odom0[1] - (s * tx + c * ty), phi1])


def ego_motion(scan, scan_phi, pred_flow, pred_cls=None, pred_reg=None, min_dist=0.5, cls_thresh=0.5, max_range=20.0,
               huber_delta=0.02, iters=4):
    """The sensor's own motion between the previous scan and this one from a canonical flow field [N,2] (cast to
    float32, the flow nets' type), as a displacement: a point now at p was at R(theta) p + u.  With pred_cls [N,1]
    (sigmoid scores) and pred_reg [N,2] the centre NMS runs first and the points of detections with a score >=
    cls_thresh stay out of the fit.  -> dict: motion [3] = (theta, u_x, u_y), ok (bool), count, rms, flow_residual
    [N,2] (the scanner-frame flow with the sensor's motion taken out: a person's own motion)."""
    tab = _table_for(scan_phi)
    ranges = _to_dev(scan, torch.float32).reshape(1, -1)
    gate = {}
    if pred_cls is not None and pred_reg is not None:
        _, dc, num, inst, _ = _nms(ranges, tab, pred_cls, pred_reg, min_dist)
        gate = dict(instance_mask=inst, num_det=num, det_cls=dc, cls_thresh=cls_thresh)
    res = ops.ego_motion(ranges, tab, _to_dev(pred_flow, torch.float32).reshape(1, -1, 2), max_range=max_range,
                         huber_delta=huber_delta, iters=iters, **gate)
    return {"motion": _host(res.motion), "ok": bool(res.ok[0].item()), "count": int(res.count[0].item()),
            "rms": float(res.rms[0].item()), "flow_residual": _host(res.flow_residual)}


def scan_match(scan_prev, scan_cur, scan_phi, pred_cls=None, pred_reg=None, **kw):
    """The sensor's own motion between the previous scan and this one from the two scans alone (``ops.scan_match``, a
    point-to-line ICP; no flow net), as a displacement: a point now at p was at R(theta) p + u.  With pred_cls [N,1]
    (sigmoid scores) and pred_reg [N,2] of the current scan the centre NMS runs first and the points of detections
    with a score >= cls_thresh do not vote.  ``kw``: min_dist (0.5, the NMS distance) and the settings of
    ``ops.scan_match`` (init [3], cls_thresh, max_range, window, gate, max_gap, huber_delta, iters, eps_theta, eps_u,
    min_pivot).  -> dict: motion [3] =
    (theta, u_x, u_y), ok (bool), count, rms, iters_used, obs, corr [N] and flow_residual [N,2]."""
    tab = _table_for(scan_phi)
    prev = _to_dev(scan_prev, torch.float32).reshape(1, -1)
    cur = _to_dev(scan_cur, torch.float32).reshape(1, -1)
    kw = dict(kw)
    min_dist = kw.pop("min_dist", 0.5)
    if kw.get("init") is not None:
        kw["init"] = _to_dev(kw["init"], torch.float64).reshape(1, 3)
    if pred_cls is not None and pred_reg is not None:
        _, dc, num, inst, _ = _nms(cur, tab, pred_cls, pred_reg, min_dist)
        kw.update(instance_mask=inst, num_det=num, det_cls=dc)
    res = ops.scan_match(prev, cur, tab, **kw)
    return {"motion": _host(res.motion), "ok": bool(res.ok[0].item()), "count": int(res.count[0].item()),
            "rms": float(res.rms[0].item()), "iters_used": int(res.iters_used[0].item()),
            "obs": float(res.obs[0].item()), "corr": _host(res.corr), "flow_residual": _host(res.flow_residual)}


# ------------------------------------------------------------------ A6
def _csr_one(dets, cls_ids):
    d = np.asarray(dets, dtype=np.float64).reshape(-1, 2)
    return ops.DetCSR.from_numpy(np.array([0, len(d)], dtype=np.int32), d,
                                 np.asarray(cls_ids, dtype=np.uint8).reshape(-1), _device())


def closest_detection(scan, scan_phi, dets, radii):
    """:232-256.  `radii` may differ per detection: detections are grouped into at
    most three radius classes (the reference only ever uses three)."""
    if len(dets) == 0:
        return np.zeros_like(scan, dtype=int)
    assert len(dets) == len(radii), "Need to give a radius for each detection!"
    uniq = sorted(set(float(r) for r in radii))
    assert len(uniq) <= 3, "at most three distinct radii are supported per call"
    cls_ids = [uniq.index(float(r)) for r in radii]
    rad3 = (uniq + [uniq[-1]] * 3)[:3]
    out = ops.scan_preprocess(_to_dev(scan, torch.float32).reshape(1, -1), _table_for(scan_phi),
                              dets=_csr_one(dets, cls_ids), assoc_radius=rad3, want=("closest",))
    return out["closest"][0].cpu().numpy()


def get_regression_target(scan, scan_phi, wcs, was, wps, radius_wc=0.6, radius_wa=0.4, radius_wp=0.35,
                          label_wc=1, label_wa=2, label_wp=3, pedestrian_only=False):
    """:147-185 -> (target_cls int64 [N], target_reg float32 [N,2])."""
    if pedestrian_only:
        dets, cls_ids = list(wps), [2] * len(wps)
        labels = (1, 1, 1)
    else:
        dets = list(wcs) + list(was) + list(wps)
        cls_ids = [0] * len(wcs) + [1] * len(was) + [2] * len(wps)
        labels = (label_wc, label_wa, label_wp)
    out = ops.scan_preprocess(_to_dev(scan, torch.float32).reshape(1, -1), _table_for(scan_phi),
                              dets=_csr_one(dets, cls_ids), assoc_radius=(radius_wc, radius_wa, radius_wp),
                              labels=labels, want=("target_cls", "target_reg"))
    return out["target_cls"][0].cpu().numpy(), out["target_reg"][0].cpu().numpy()


# ------------------------------------------------------------------ A8
def scans_to_cutout(scans, scan_phi, stride=1, centered=True, fixed=False, window_width=1.66,
                    window_depth=1.0, num_cutout_pts=48, padding_val=29.99, area_mode=False):
    """:259-334.  scans (T,N) -> (N/stride, T, P) float32; a leading batch axis
    ([B,T,N] -> [B,N/stride,T,P]) is accepted."""
    tensor_in = _is_t(scans)
    s = _to_dev(scans, torch.float32)
    batched = s.dim() == 3
    out = ops.cutout(s if batched else s[None], _table_for(scan_phi), stride=stride, centered=centered,
                     fixed=fixed, window_width=window_width, window_depth=window_depth,
                     num_cutout_pts=num_cutout_pts, padding_val=padding_val, area_mode=area_mode)
    out = out if batched else out[0]
    return out if tensor_in else out.cpu().numpy()


def scans_to_polar_grid(scans, min_range=0.0, max_range=30.0, range_bin_size=1.0, tsdf_clip=1.0,
                        normalize=True):
    """:492-531.  scans (T,N) -> (T, R, N) float32 TSDF columns; a leading batch axis is accepted."""
    tensor_in = _is_t(scans)
    s = _to_dev(scans, torch.float32)
    batched = s.dim() == 3
    out = ops.polar_grid(s if batched else s[None], min_range, max_range, range_bin_size, tsdf_clip, normalize)
    out = out if batched else out[0]
    return out if tensor_in else out.cpu().numpy()


def scans_to_cutout_torch(scans, scan_phi, stride=1, centered=True, fixed=False, window_width=1.66,
                          window_depth=1.0, num_cutout_pts=48, padding_val=29.99, area_mode=False):
    """:337-420.  The reference's torch twin does its index math in float32 and
    disagrees with its own NumPy version; this follows the NumPy (float64) one."""
    return scans_to_cutout(scans, scan_phi, stride, centered, fixed, window_width, window_depth,
                           num_cutout_pts, padding_val, area_mode)


# ------------------------------------------------------------------ A11
def nms_predicted_center(scan_grid, phi_grid, pred_cls, pred_reg, min_dist=0.5):
    """:535-571 -> (det_xys [M,2], det_cls [M,1], instance_mask [N] int32)."""
    xy, dc, num, inst, dtype = _nms(_to_dev(scan_grid, torch.float32).reshape(1, -1), _table_for(phi_grid), pred_cls,
                                    pred_reg, min_dist)
    m = int(num[0].item())
    return xy[0, :m].cpu().numpy(), dc[0, :m].cpu().numpy().reshape(-1, 1).astype(dtype), _host(inst)


def flow_to_hsv(flow):
    """:574-584.  Flow vectors [..., 2] -> RGB colours [..., 3] (float64): hue from the direction, saturation from
    min(|flow|, 0.1) / 0.1, value 1.  The polar conversion is the HIP ``xy_to_rphi``; the HSV -> RGB step repeats
    ``colorsys.hsv_to_rgb``'s arithmetic for all vectors at once instead of one Python call per point."""
    fl = flow.detach().cpu().numpy() if _is_t(flow) else np.asarray(flow)
    r, phi = xy_to_rphi(np.ascontiguousarray(fl[..., 0], dtype=np.float64), np.ascontiguousarray(fl[..., 1], dtype=np.float64))
    h = (phi + 2.0 * np.pi) / np.pi / 2
    sat = np.minimum(r, 0.1) / 0.1
    v = np.ones_like(h)
    sector = (h * 6.0).astype(np.int64)             # int(): truncation; h > 0 here
    f = h * 6.0 - sector
    p, q, t = v * (1.0 - sat), v * (1.0 - sat * f), v * (1.0 - sat * (1.0 - f))
    sector = sector % 6
    table = np.stack([np.stack(c, axis=-1) for c in ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))])
    rgb = np.take_along_axis(table, sector[None, ..., None], axis=0)[0]
    return np.where((sat == 0.0)[..., None], v[..., None], rgb)


def person_flow(scan, scan_phi, pred_cls, pred_reg, pred_flow, odom1=None, odom0=None, min_dist=0.5, cls_thresh=0.5):
    """The per-person result of depracted_scripts/infer_person_flow.py:134-157 for one scan: the centre NMS, then
    in ONE launch the scanner-frame flow (``canonical_to_global_flow_torch``), its world-frame form
    ``np.matmul(flow, odom_rot.T) + (odom1 - odom0)[:2]``, the colour code and, per detection, the world centre
    ``np.matmul(dets_xy, odom_rot.T) + odom1[:2]`` and the mean flow / mean colour of its points.

    scan [N], pred_cls [N,1] (sigmoid scores), pred_reg [N,2], pred_flow [N,2] canonical (cast to float32, the flow
    nets' type); odom1 / odom0: the sensor's world (x, y, phi) at this scan and at the previous one.  Without odom1
    everything stays in the scanner frame, without odom0 no translation is added to the flow.
    -> dict: dets_xy_world [M,2], dets_cls [M,1], person_flow [M,2], person_rgb [M,3], count [M], valid [M] (bool:
    ``dets_cls >= cls_thresh``, the detections the reference draws with an arrow), instance_mask [N], flow_world
    [N,2], rgb [N,3].  A detection whose points all went to later detections has count 0 and NaN means."""
    tab = _table_for(scan_phi)
    xy, dc, num, inst, dtype = _nms(_to_dev(scan, torch.float32).reshape(1, -1), tab, pred_cls, pred_reg, min_dist)
    rot, trans, flow_trans = _pose_terms(None if odom1 is None else np.asarray(odom1, dtype=np.float64)[None],
                                         None if odom0 is None else np.asarray(odom0, dtype=np.float64)[None])
    out = ops.person_flow(_to_dev(pred_flow, torch.float32).reshape(1, -1, 2), tab, inst, num, xy, dc,
                          _to_dev(rot, torch.float32), _to_dev(trans, torch.float64),
                          _to_dev(flow_trans, torch.float64), cls_thresh)
    m = int(num[0].item())
    return {"dets_xy_world": _host(out.det_xy_world)[:m], "dets_cls": _host(dc)[:m].reshape(-1, 1).astype(dtype),
            "person_flow": _host(out.det_flow)[:m], "person_rgb": _host(out.det_rgb)[:m],
            "count": _host(out.det_count)[:m], "valid": _host(out.det_valid)[:m].astype(bool),
            "instance_mask": _host(inst), "flow_world": _host(out.flow_world), "rgb": _host(out.rgb)}


class PersonTracker:
    """Person tracks over the results of ``person_flow``, scan after scan (``ops.track_update``, one launch per scan;
    the reference has no tracker).  ``tracker = PersonTracker(max_tracks=64, gate=0.5, ...)`` with the settings of
    ``ops.track_update``; ``ids, tracks = tracker.update(result)`` per scan, ``tracker.reset()`` between sequences.

    ``update(result)``: the dict ``person_flow`` returns (dets_xy_world [M,2], person_flow [M,2], valid [M] and, when
    present, instance_mask [N]), NumPy in and NumPy out.  -> ids [M] int32, the track id of every detection (0: not
    valid, or no slot was free), and the live tracks as a dict of arrays in slot order: id, xy [T,2], velocity [T,2]
    (metres per scan), cov [T,3], hits, misses, age, confirmed and det (the detection's row, -1 when missed); with an
    instance_mask also point_track [N], the track id of every scan point."""

    def __init__(self, max_tracks=64, **settings):
        self.max_tracks, self.settings = int(max_tracks), _stage_kw(ops.track_update, "tracks", settings)
        self._persistent = self._last = None

    def reset(self):
        self._persistent = self._last = None

    def update(self, result):
        xy = np.asarray(result["dets_xy_world"], dtype=np.float64).reshape(-1, 2)
        m = len(xy)
        inst = result.get("instance_mask")
        n = max(m, 1) if inst is None else len(inst)
        dev = _device()
        pad = lambda a, dtype, *w: torch.from_numpy(np.concatenate(
            [np.asarray(a, dtype=dtype).reshape((m,) + w), np.zeros((n - m,) + w, dtype)])[None]).to(dev)
        state = ops.track_buffers(1, self.max_tracks, n, dev)
        if self._persistent is not None:
            state = state._replace(**self._persistent)
        ops.track_update(pad(xy, np.float64, 2), pad(result["person_flow"], np.float64, 2),
                         pad(result["valid"], np.uint8), torch.full((1,), m, dtype=torch.int32, device=dev),
                         torch.zeros((1, n), dtype=torch.int32, device=dev) if inst is None else
                         _to_dev(inst, torch.int32).reshape(1, n), state, **self.settings)
        self._persistent = {k: getattr(state, k) for k in ops.TrackState.persistent}
        self._last = state                                     # on the device, for ``TrackMap.update``
        h = {k: getattr(state, k)[0].cpu().numpy() for k in state._fields}
        live = np.flatnonzero(h["track_id"])
        tracks = {"id": h["track_id"][live], "xy": h["track_state"][live, :2], "velocity": h["track_state"][live, 2:],
                  "cov": h["track_cov"][live], "hits": h["track_hits"][live], "misses": h["track_misses"][live],
                  "age": h["track_age"][live], "confirmed": h["track_confirmed"][live].astype(bool),
                  "det": h["track_det"][live]}
        if inst is not None:
            tracks["point_track"] = h["point_track"]
        return h["det_track"][:m], tracks


class PersonMotion:
    """Per-person displacement from the scans alone, scan after scan (``ops.person_motion``, one launch per scan; the
    reference has nothing of the kind): the world-frame centroid of every detection's own scan points, paired with the
    previous scan's centroids by a strict mutual-nearest rule.  ``pm = PersonMotion(scan_phi, reach=0.5, ...)`` with
    the settings of ``ops.person_motion`` (``cls_thresh``, ``max_range``, ``reach``, ``min_points``) and min_dist (0.5,
    the NMS distance); ``res = pm.update(scan, pred_cls, pred_reg, odom)`` per scan, ``pm.reset()`` between sequences.

    ``update``: NumPy in and NumPy out.  scan [N], pred_cls [N,1] (sigmoid scores), pred_reg [N,2]; odom = the
    sensor's world (x, y, phi) at this scan (None: scanner frame).  The centre NMS runs first.  -> dict with the
    per-detection keys of ``person_flow`` -- dets_xy_world [M,2], dets_cls [M,1], person_flow [M,2] (the displacement
    since the previous scan, NaN without a partner), count [M], valid [M] -- and centre [M,2], prev [M] (the partner's
    row in the previous result or -1) and instance_mask [N]; ``PersonTracker.update`` takes it as it is."""

    def __init__(self, scan_phi, **kw):
        self._tab = _table_for(scan_phi)
        self._n = self._tab.numel() // 3
        self._min_dist = kw.pop("min_dist", 0.5)
        self._kw = _stage_kw(ops.person_motion, "person_motion", kw)
        self._state = ops.person_motion_state(1, self._n, self._tab.device)

    def reset(self):
        ops.person_motion_reset(self._state)

    def update(self, scan, pred_cls, pred_reg, odom=None):
        cur = _to_dev(scan, torch.float32).reshape(1, -1)
        xy, dc, num, inst, dtype = _nms(cur, self._tab, pred_cls, pred_reg, self._min_dist)
        rot, trans, _ = _pose_terms(None if odom is None else np.asarray(odom, dtype=np.float64)[None])
        out = ops.person_motion(cur, self._tab, inst, num, xy, dc, _to_dev(rot, torch.float32),
                                _to_dev(trans, torch.float64), self._state, **self._kw)
        m = int(num[0].item())
        return {"dets_xy_world": _host(out.det_xy_world)[:m], "dets_cls": _host(dc)[:m].reshape(-1, 1).astype(dtype),
                "person_flow": _host(out.det_flow)[:m], "count": _host(out.det_count)[:m],
                "valid": _host(out.det_valid)[:m].astype(bool), "centre": _host(out.det_centre)[:m],
                "prev": _host(out.det_prev)[:m], "instance_mask": _host(inst)}


class KeyframeOdometry:
    """The sensor's pose from its scans alone, scan after scan, without the drift of composing one scan-to-scan fit
    per scan (``ops.keyframe_match``, one launch per scan; the reference has no scan matcher): every scan is matched
    against a keyframe that stays fixed until the sensor has moved away from it.  ``odo = KeyframeOdometry(scan_phi,
    key_dist=0.3, ...)`` with the settings of ``ops.keyframe_match`` and min_dist (0.5, the NMS distance);
    ``res = odo.update(scan, pred_cls, pred_reg)`` per scan, ``odo.reset(pose)`` between sequences.

    ``update``: NumPy in and NumPy out.  With pred_cls [N,1] (sigmoid scores) and pred_reg [N,2] the centre NMS runs
    first: the points of detections with a score >= cls_thresh do not vote and never become vertices of a keyframe.
    -> dict: pose [3] = (x, y, phi), motion [3] = (theta, u_x, u_y) against the keyframe, ok (bool; False on the first
    scan, which only becomes the keyframe), count, rms, iters_used, obs, key_replaced (bool), key_age, key_misses,
    key_pose [3], corr [N] and flow_residual [N,2]."""

    def __init__(self, scan_phi, **kw):
        self._setup(scan_phi, kw)
        self._state = ops.keyframe_buffers(1, self._n, self._tab.device)

    def _setup(self, scan_phi, kw):
        self._tab = _table_for(scan_phi)
        self._n = self._tab.numel() // 3
        self._min_dist = kw.pop("min_dist", 0.5)
        self._kw = _stage_kw(ops.keyframe_match, "keyframe", kw)

    _reset, _match = staticmethod(ops.keyframe_reset), staticmethod(ops.keyframe_match)

    def reset(self, pose=None):
        self._reset(self._state, pose)

    def update(self, scan, pred_cls=None, pred_reg=None):
        return self._step(scan, pred_cls, pred_reg)[1]

    def _step(self, scan, pred_cls, pred_reg):
        """-> the outputs on the device and the dict ``KeyframeOdometry.update`` returns."""
        cur = _to_dev(scan, torch.float32).reshape(1, -1)
        gate = {}
        if pred_cls is not None and pred_reg is not None:
            _, dc, num, inst, _ = _nms(cur, self._tab, pred_cls, pred_reg, self._min_dist)
            gate = dict(instance_mask=inst, num_det=num, det_cls=dc)
        res = self._match(cur, self._tab, self._state, **gate, **self._kw)
        s = self._state
        return res, {"pose": _host(s.pose), "motion": _host(res.motion), "ok": bool(res.ok[0].item()),
                     "count": int(res.count[0].item()), "rms": float(res.rms[0].item()),
                     "iters_used": int(res.iters_used[0].item()), "obs": float(res.obs[0].item()),
                     "key_replaced": bool(res.key_replaced[0].item()), "key_age": int(s.key_age[0].item()),
                     "key_misses": int(s.key_misses[0].item()), "key_pose": _host(s.key_pose), "corr": _host(res.corr),
                     "flow_residual": _host(res.flow_residual)}


class KeyframeMapOdometry(KeyframeOdometry):
    """``KeyframeOdometry`` with a ring of ``keys`` keyframes (``ops.keyframe_map_match``, one launch per scan): a
    sensor that comes back to a place it has a keyframe of switches to that keyframe, and the next match re-anchors
    the pose on it -- the drift of the way round is dropped.  ``odo = KeyframeMapOdometry(scan_phi, keys=16,
    revisit=0.5, key_dist=0.3, ...)`` with the settings of ``ops.keyframe_map_match`` and min_dist (0.5, the NMS
    distance); ``res = odo.update(scan, pred_cls, pred_reg)`` per scan, ``odo.reset(pose)`` between sequences.

    ``update``: NumPy in and NumPy out, as ``KeyframeOdometry.update``.  -> its dict (key_pose [3] is the active
    slot's) with key_switched (bool) and key_slot, the active slot after the step."""

    def __init__(self, scan_phi, keys=16, revisit=0.5, **kw):
        self._setup(scan_phi, kw)
        if not 0.0 <= float(revisit) <= 1.0:
            raise ValueError("revisit must be in [0, 1]")
        self._kw = dict(kw, revisit=float(revisit))
        self._state = ops.keyframe_map_buffers(1, self._n, keys, self._tab.device)

    _reset, _match = staticmethod(ops.keyframe_map_reset), staticmethod(ops.keyframe_map_match)

    def update(self, scan, pred_cls=None, pred_reg=None):
        res, d = self._step(scan, pred_cls, pred_reg)
        slot = int(res.key_slot[0].item())
        d.update(key_switched=bool(res.key_switched[0].item()), key_slot=slot,
                 key_pose=self._state.key_pose[0, slot].cpu().numpy())
        return d


class OccupancyGrid:
    """An occupancy grid map of what one sensor has seen, scan after scan (``ops.grid_map_update``, two launches per
    scan; the reference has nothing of the kind): an int16 log-odds grid of ``size`` x ``size`` cells (or ``size`` =
    (H, W); multiples of 64) of ``res`` metres, kept on the device.  ``og = OccupancyGrid(scan_phi, res=0.1, size=512,
    ...)`` with the settings of ``ops.grid_map_update`` (``cls_thresh``, ``max_range``, ``tol``, ``hit``, ``miss``,
    ``lo``, ``hi``, ``free_thresh``) and min_dist (0.5, the NMS distance); ``res = og.update(scan, odom, pred_cls,
    pred_reg)`` per scan, ``og.reset(origin)`` between sequences.

    ``update``: NumPy in and NumPy out.  scan [N]; odom = the sensor's world (x, y, phi) at this scan (None: the world
    origin).  With pred_cls [N,1] (sigmoid scores) and pred_reg [N,2] the centre NMS runs first and the points of
    detections with a score >= cls_thresh are not burned in.  -> dict: point_cell [N], point_mark [N] (bool),
    point_prior [N], and with predictions det_points [M], det_free [M], dets_cls [M,1] and instance_mask [N].
    ``reset(origin)``: every cell unknown; origin [2] = the world position of the grid's lower corner -- by default the
    next update puts its pose in the middle of the grid.  ``logodds`` is the grid [H,W] int16 on the host,
    ``probability(unit)`` the occupancy probability of a count worth ``unit`` nat.  ``localize(scan, odom, ...)``
    corrects a pose against the grid as it stands (``ops.grid_match``) without updating it and ``refine(scan, odom,
    ...)`` fits it below the size of a cell (``ops.grid_refine``), the caller updating afterwards; ``cast(scan, odom, ...)``
    ray-casts the grid as it stands along every beam (``ops.grid_cast``), to be called before the scan's ``update``;
    ``novel_segments(scan, odom, ...)`` does that and groups the NOVEL points into detections (``ops.novel_segments``);
    ``merged_detections(scan, odom, ...)`` does that and merges them with the NMS's (``ops.merge_detections``).
    ``scroll=dict(margin=...)`` (None: the grid stays where ``reset`` put it): the grid follows the sensor
    (``ops.grid_scroll``, two more launches in front of ``update`` and ``localize``): within ``margin`` cells of a border
    (None: a quarter of the shorter side in whole tiles) it is shifted by whole tiles of 64 cells so that the sensor
    stands on the middle tile again.  The result dicts then hold ``shift`` [2] = this call's shift in tiles (x, y),
    ``offset`` is the shift since the last reset [2] and ``origin`` moves with it.
    ``store=dict(slots=64)`` (needs ``scroll``; None: what leaves the grid is gone): a store of ``slots`` tiles behind the
    grid (``ops.grid_scroll_store`` in the place of ``ops.grid_scroll``, three launches): a tile that scrolls out and is
    not all unknown is kept, first in free slots and then in the one written longest ago, and a tile that scrolls in
    comes back from there bit for bit, so a return to a mapped place finds its map.  The result dicts then also hold
    ``store_counts`` [4] = this call's (restored, stored, evicted, dropped) tiles, ``store_tiles`` is the number of
    tiles in the store, and ``reset`` empties it."""

    def __init__(self, scan_phi, res=0.1, size=512, scroll=None, store=None, **kw):
        # the settings first: a wrong one raises before anything touches the device
        self._min_dist = kw.pop("min_dist", 0.5)
        self._scroll_kw = None if scroll is None else dict(_stage_kw(ops.grid_scroll, "scroll", dict(scroll), "res"))
        self._store = None
        if store is not None:
            if scroll is None:
                raise ValueError("store keeps what scroll moves out of the grid: give both")
            store = dict({"slots": 64}, **store)
            if set(store) != {"slots"}:
                raise ValueError("unknown store settings: %s" % sorted(set(store) - {"slots"}))
            slots = ops.grid_store_slots(store["slots"])
        _stage_kw(ops.grid_map_update, "grid_map", kw, "res")
        self.res = float(res)
        if not self.res > 0.0:
            raise ValueError("res must be > 0")
        self.shape = ops.grid_shape(size)
        if self._scroll_kw is not None:
            ops.grid_scroll_margin(*self.shape, self._scroll_kw.get("margin"))
        self._kw = kw
        self._tab = _table_for(scan_phi)
        self._n = self._tab.numel() // 3
        self._state = ops.grid_map_state(1, *self.shape, self._tab.device)
        self._centre = True
        self._last = None                                      # (outputs, instance_mask, num_det) of the last update
        if self._scroll_kw is not None:
            self._scroll = ops.grid_scroll_state(1, *self.shape, self._tab.device)
            self._scroll_out = ops.grid_scroll_buffers(1, self._tab.device)
        if store is not None:
            self._store = ops.grid_store_state(1, *self.shape, slots, self._tab.device)
            self._scroll_out = ops.grid_scroll_store_buffers(1, self._tab.device)

    def reset(self, origin=None):
        self._reset(origin)
        self._centre = origin is None

    def _reset(self, origin):
        ops.grid_map_reset(self._state, origin)
        if self._scroll_kw is not None:
            ops.grid_scroll_reset(self._scroll, self._state)
        if self._store is not None:
            ops.grid_store_reset(self._store)

    def _scrolled(self, trans):
        """With ``scroll``: the grid follows the sensor at trans [1,2] (device) -> {"shift": [2]}, with ``store`` also
        "store_counts": [4]; else {}."""
        if self._scroll_kw is None:
            return {}
        if self._store is not None:
            out = ops.grid_scroll_store(trans, self._state, self._scroll, self._store, res=self.res, out=self._scroll_out,
                                        **self._scroll_kw)
            return {"shift": _host(out.shift), "store_counts": _host(out.counts)}
        out = ops.grid_scroll(trans, self._state, self._scroll, res=self.res, out=self._scroll_out, **self._scroll_kw)
        return {"shift": _host(out.shift)}

    def update(self, scan, odom=None, pred_cls=None, pred_reg=None):
        cur = _to_dev(scan, torch.float32).reshape(1, -1)
        gate, dc = {}, None
        if pred_cls is not None and pred_reg is not None:
            _, dc, num, inst, dtype = _nms(cur, self._tab, pred_cls, pred_reg, self._min_dist)
            gate = dict(instance_mask=inst, num_det=num, det_cls=dc)
        rot, trans, _ = _pose_terms(None if odom is None else np.asarray(odom, dtype=np.float64)[None])
        if self._centre:                                       # the first pose of a sequence in the middle of the grid
            self._reset(trans[0] - 0.5 * self.res * np.array(self.shape[::-1], dtype=np.float64))
            self._centre = False
        trans = _to_dev(trans, torch.float64)
        shift = self._scrolled(trans)
        out = ops.grid_map_update(cur, self._tab, _to_dev(rot, torch.float32), trans, self._state, res=self.res, **gate,
                                  **self._kw)
        result = dict(shift, point_cell=_host(out.point_cell), point_mark=_host(out.point_mark).astype(bool),
                      point_prior=_host(out.point_prior))
        self._last = None if dc is None else (out, inst, num)  # on the device, for ``TrackMap.update``
        if dc is not None:
            m = int(num[0].item())
            result.update(det_points=_host(out.det_points)[:m], det_free=_host(out.det_free)[:m],
                          dets_cls=_host(dc)[:m].reshape(-1, 1).astype(dtype), instance_mask=_host(inst))
        return result

    def localize(self, scan, odom, pred_cls=None, pred_reg=None, **settings):
        """The pose ``odom`` = (x, y, phi) corrected against the grid as it stands (``ops.grid_match``, two launches;
        ``settings``: its ``reach``, ``rotations``, ``rot_step``, ``min_points``, ``min_score``, ``min_gain``).  The
        grid is not updated.  With predictions the centre NMS runs first and people's points do not vote.
        -> (the corrected (x, y, phi) [3], dict of best [3] = (rotation steps, dy, dx in cells), score [2] = (the best
        candidate's, the given pose's), votes, ok, moved (bool) and correction [3])."""
        _stage_kw(ops.grid_match, "grid_match", settings, "res", "cls_thresh", "max_range")
        cur = _to_dev(scan, torch.float32).reshape(1, -1)
        gate = {}
        if pred_cls is not None and pred_reg is not None:
            _, dc, num, inst, _ = _nms(cur, self._tab, pred_cls, pred_reg, self._min_dist)
            gate = dict(instance_mask=inst, num_det=num, det_cls=dc)
        pose = np.asarray(odom, dtype=np.float64).reshape(1, 3)
        rot, trans, _ = _pose_terms(pose)
        pose, trans = _to_dev(pose, torch.float64), _to_dev(trans, torch.float64)
        shift = self._scrolled(trans)
        shared = {k: self._kw[k] for k in ("cls_thresh", "max_range") if k in self._kw}
        out = ops.grid_match(cur, self._tab, _to_dev(rot, torch.float32), trans, pose, self._state, res=self.res,
                             **gate, **shared, **settings)
        return _host(pose), dict(shift, best=_host(out.best), score=_host(out.score), votes=int(out.votes[0].item()),
                                 ok=bool(out.ok[0].item()), moved=bool(out.moved[0].item()),
                                 correction=_host(out.correction))

    def refine(self, scan, odom, pred_cls=None, pred_reg=None, **settings):
        """The pose ``odom`` = (x, y, phi) fitted to the grid as it stands below the size of a cell (``ops.grid_refine``,
        one launch; ``settings``: its ``cap``, ``iters``, ``min_points``, ``min_pivot``, ``max_shift``, ``max_turn``,
        ``eps_shift``, ``eps_turn``).  The grid is not updated: the caller enters the scan at the returned pose
        afterwards.  With predictions the centre NMS runs first and people's points do not vote.
        -> (the refined (x, y, phi) [3], dict of correction [3], score [2] = the mean interpolated grid value (before,
        after), obs, votes, count, iters_used, ok and moved (bool))."""
        _stage_kw(ops.grid_refine, "grid_refine", settings, "res", "cls_thresh", "max_range")
        cur = _to_dev(scan, torch.float32).reshape(1, -1)
        gate = {}
        if pred_cls is not None and pred_reg is not None:
            _, dc, num, inst, _ = _nms(cur, self._tab, pred_cls, pred_reg, self._min_dist)
            gate = dict(instance_mask=inst, num_det=num, det_cls=dc)
        pose = np.asarray(odom, dtype=np.float64).reshape(1, 3)
        rot, trans, _ = _pose_terms(pose)
        pose, trans = _to_dev(pose, torch.float64), _to_dev(trans, torch.float64)
        shift = self._scrolled(trans)
        shared = {k: self._kw[k] for k in ("cls_thresh", "max_range") if k in self._kw}
        out = ops.grid_refine(cur, self._tab, _to_dev(rot, torch.float32), trans, pose, self._state, res=self.res,
                              **gate, **shared, **settings)
        return _host(pose), dict(shift, correction=_host(out.correction), score=_host(out.score),
                                 obs=float(out.obs[0].item()), votes=int(out.votes[0].item()),
                                 count=int(out.count[0].item()), iters_used=int(out.iters_used[0].item()),
                                 ok=bool(out.ok[0].item()), moved=bool(out.moved[0].item()))

    def cast(self, scan, odom=None, pred_cls=None, pred_reg=None, **settings):
        """The scan the grid predicts at the pose ``odom`` = (x, y, phi), and what it says about every point of ``scan``
        (``ops.grid_cast``, two launches; ``settings``: its ``tol``, ``occ_thresh``, ``free_thresh``; ``max_range`` is
        the grid's).  The grid is not updated and is read as it stands: call this BEFORE the ``update`` of the same
        scan, which then enters the scan at the same pose (a first pose is put in the middle of the grid here as it
        would be there, and with ``scroll`` the grid scrolls here first).  With predictions the centre NMS runs first
        and the classes are also counted per detection.
        -> dict: exp_range, exp_far, free_range [N] (+inf without), exp_cell, exp_state (0 none, 1 open, 2 edge, 3
        wall, 4 outside), exp_steps [N], point_class [N] (0 none, 1 map, 2 novel, 3 through, 4 unknown), class_count
        [5], and with predictions det_novel, det_map, det_through [M], dets_cls [M,1] and instance_mask [N]."""
        return self._cast(scan, odom, pred_cls, pred_reg, _stage_kw(ops.grid_cast, "grid_cast", settings, "res",
                                                                    "max_range"))[0]

    def _cast(self, scan, odom, pred_cls, pred_reg, settings):
        """``cast`` -> (its dict, the scan [1,N] on the device, the ``ops.GridCast``, the NMS gate's keywords, the NMS's
        det_xy or None)."""
        cur = _to_dev(scan, torch.float32).reshape(1, -1)
        gate, dc, xy = {}, None, None
        if pred_cls is not None and pred_reg is not None:
            xy, dc, num, inst, dtype = _nms(cur, self._tab, pred_cls, pred_reg, self._min_dist)
            gate = dict(instance_mask=inst, num_det=num, det_cls=dc)
        rot, trans, _ = _pose_terms(None if odom is None else np.asarray(odom, dtype=np.float64)[None])
        if self._centre:                                       # as ``update``: the first pose in the middle of the grid
            self._reset(trans[0] - 0.5 * self.res * np.array(self.shape[::-1], dtype=np.float64))
            self._centre = False
        trans = _to_dev(trans, torch.float64)
        shift = self._scrolled(trans)
        shared = {k: self._kw[k] for k in ("max_range",) if k in self._kw}
        out = ops.grid_cast(cur, self._tab, _to_dev(rot, torch.float32), trans, self._state, res=self.res, **gate,
                            **shared, **settings)
        result = dict(shift, **{k: _host(getattr(out, k)) for k in out._fields if not k.startswith("det_")})
        if dc is not None:
            m = int(num[0].item())
            result.update({k: _host(getattr(out, k))[:m] for k in ("det_novel", "det_map", "det_through")},
                          dets_cls=_host(dc)[:m].reshape(-1, 1).astype(dtype), instance_mask=_host(inst))
        return result, cur, out, gate, xy

    def novel_segments(self, scan, odom=None, pred_cls=None, pred_reg=None, **settings):
        """``cast(scan, odom, ...)`` and, on its classes, the runs of NOVEL points as detections
        (``ops.novel_segments``, one more launch; ``settings``: its ``jump``, ``max_skip``, ``min_points``,
        ``max_width`` and the ``tol``, ``occ_thresh``, ``free_thresh`` of the cast; ``cls_thresh`` is the grid's).  Like
        ``cast`` it updates nothing and is to be called BEFORE the ``update`` of the same scan; it centres a first pose
        and scrolls as ``cast`` does.  With predictions ``seg_known`` says how many points of a segment the NMS's
        confident detections hold.
        -> the dict of ``cast`` and seg_instance_mask [N] (k + 1 on the points of kept segment k), seg_num (K, the kept
        segments), seg_xy [K,2] (the mean of the segment's points, sensor frame), seg_cls [K] (ones), seg_points,
        seg_first, seg_last, seg_known [K], seg_width2 [K] and seg_count [3] (segments before the filters, dropped as
        few, dropped as wide)."""
        return self._segments(scan, odom, pred_cls, pred_reg, settings)[0]

    def _segments(self, scan, odom, pred_cls, pred_reg, settings):
        """``novel_segments`` -> (its dict, the ``ops.NovelSegments``, the NMS gate's keywords, the NMS's det_xy or
        None)."""
        own = set(ops.stage_settings(ops.novel_segments)) - {"cls_thresh"}
        cast_kw = {k: v for k, v in settings.items() if k not in own}
        unknown = set(cast_kw) - (set(ops.stage_settings(ops.grid_cast)) - {"res", "max_range"})
        if unknown:
            raise ValueError("unknown novel_segments settings: %s" % sorted(unknown))
        result, cur, out, gate, xy = self._cast(scan, odom, pred_cls, pred_reg, cast_kw)
        shared = {k: self._kw[k] for k in ("cls_thresh",) if k in self._kw}
        seg = ops.novel_segments(cur, self._tab, out.point_class, **gate, **shared,
                                 **{k: v for k, v in settings.items() if k in own})
        m = int(seg.num_det[0].item())
        result.update(seg_instance_mask=_host(seg.instance_mask), seg_num=m, seg_count=_host(seg.seg_count),
                      **{name: _host(getattr(seg, f))[:m] for name, f in (
                          ("seg_xy", "det_xy"), ("seg_cls", "det_cls"), ("seg_points", "det_count"),
                          ("seg_first", "det_first"), ("seg_last", "det_last"), ("seg_width2", "det_width2"),
                          ("seg_known", "det_known"))})
        return result, seg, gate, xy

    def merged_detections(self, scan, odom=None, pred_cls=None, pred_reg=None, **settings):
        """``novel_segments(scan, odom, ...)`` and its segments merged with the NMS's detections of the same call
        (``ops.merge_detections``, one more launch; ``settings``: its ``absorb_pct`` and the settings of
        ``novel_segments``; ``cls_thresh`` is the grid's).  Like ``cast`` it updates nothing and is to be called BEFORE
        the ``update`` of the same scan.  Without predictions the merged record is the segments'.
        -> the dict of ``novel_segments`` and merged_instance_mask [N], merged_num (M, the merged rows), merged_xy [M,2],
        merged_cls [M], merged_points [M], merged_src [M] (1 the NMS's, 2 a segment), merged_row [M] (the row in its own
        record), seg_row [K] (per segment its merged row; -1 absorbed, -2 dropped) and merge_count [4] (the NMS's rows,
        appended, absorbed, dropped)."""
        own = set(ops.stage_settings(ops.merge_detections)) - {"cls_thresh"}
        result, seg, gate, xy = self._segments(scan, odom, pred_cls, pred_reg,
                                               {k: v for k, v in settings.items() if k not in own})
        shared = {k: self._kw[k] for k in ("cls_thresh",) if k in self._kw}
        out = ops.merge_detections(*seg[:4], **gate, **({} if xy is None else dict(det_xy=xy)), **shared,
                                   **{k: v for k, v in settings.items() if k in own})
        m = int(out.num_det[0].item())
        result.update(merged_instance_mask=_host(out.instance_mask), merged_num=m,
                      seg_row=_host(out.b_row)[:result["seg_num"]], merge_count=_host(out.merge_count),
                      **{name: _host(getattr(out, f))[:m] for name, f in (
                          ("merged_xy", "det_xy"), ("merged_cls", "det_cls"), ("merged_points", "det_points"),
                          ("merged_src", "det_src"), ("merged_row", "det_row"))})
        return result

    @property
    def origin(self):
        return _host(self._state.origin)

    @property
    def offset(self):
        """The shift since the last reset in tiles of 64 cells [2] = (x, y); zeros without ``scroll``."""
        return _host(self._scroll.offset) if self._scroll_kw is not None else np.zeros(2, np.int32)

    @property
    def store_tiles(self):
        """The tiles the store holds; 0 without ``store``."""
        return int((self._store.store_stamp != 0).sum().item()) if self._store is not None else 0

    @property
    def logodds(self):
        return _host(self._state.grid)

    def probability(self, unit=0.05):
        return 1.0 / (1.0 + np.exp(-float(unit) * self.logodds.astype(np.float64)))


class TrackMap:
    """What the occupancy grid says about every track, scan after scan (``ops.track_map``, one launch per scan; the
    reference has nothing of the kind).  ``tm = TrackMap(max_tracks=64, occ_thresh=17, ...)`` with the settings of
    ``ops.track_map``; ``res = tm.update(tracker, grid)`` per scan, ``tm.reset()`` between sequences.

    ``update(tracker, grid)``: a ``PersonTracker`` (of the same ``max_tracks``) and an ``OccupancyGrid`` after their own
    ``update`` of this scan -- the tracker's with a result that holds the scan's instance_mask (``PersonMotion.update``
    and ``person_flow`` give one), the grid's with the same predictions, so that both speak of the same detection rows.
    NumPy out.  -> dict: the live tracks in slot order as arrays id, cls (0 undecided, 1 free-standing, 2 unsupported,
    3 background), points, free, occ (the three sums), scans, moved (bool), start [T,2]; det_class [M] per detection,
    point_class [N] per scan point and class_count [4]."""

    def __init__(self, max_tracks=64, **settings):
        self.max_tracks, self.settings = int(max_tracks), _stage_kw(ops.track_map, "track_map", settings)
        self._state = None

    def reset(self):
        self._state = None

    def update(self, tracker, grid):
        tracks, seen = getattr(tracker, "_last", None), getattr(grid, "_last", None)
        if tracks is None or seen is None:
            raise ValueError("update the tracker and the grid (with predictions) for this scan first")
        out, inst, num = seen
        if tracks.track_id.shape[1] != self.max_tracks or tracks.det_track.shape[1] != inst.shape[1]:
            raise ValueError("the tracker must have max_tracks = %d and be updated with the scan's instance_mask"
                             % self.max_tracks)
        if self._state is None:
            self._state = ops.track_map_state(1, self.max_tracks, inst.device)
        res = ops.track_map(tracks, out, inst, num, self._state, **self.settings)
        ids, m = _host(tracks.track_id), int(num[0].item())
        live = np.flatnonzero(ids)
        h = {k: _host(t) for k, t in zip(self._state._fields, self._state)}
        return {"id": ids[live], "cls": _host(res.track_class)[live], "points": h["ev_points"][live],
                "free": h["ev_free"][live], "occ": h["ev_occ"][live], "scans": h["ev_scans"][live],
                "moved": h["ev_moved"][live].astype(bool), "start": h["ev_start"][live],
                "det_class": _host(res.det_class)[:m], "point_class": _host(res.point_class),
                "class_count": _host(res.class_count)}


def _pose_terms(odom1, odom0=None, batch=1):
    """Host side of ``person_flow`` for B sensors at once: (rot [B,2,2] float32, trans [B,2], flow_trans [B,2]) of the
    poses odom1 [B,3] = (x, y, phi) and the previous ones odom0, as infer_person_flow.py:114-117,145-146 forms them
    (rot[b] has the bits of ``_phi_to_rotation_matrix(odom1[b, 2])``).  None: identity / zeros for `batch` sensors."""
    if odom1 is None:
        return np.tile(np.eye(2, dtype=np.float32), (batch, 1, 1)), np.zeros((batch, 2)), np.zeros((batch, 2))
    odom1 = np.asarray(odom1, dtype=np.float64).reshape(-1, 3)
    c, s = np.cos(odom1[:, 2]), np.sin(odom1[:, 2])
    rot = np.stack([c, -s, s, c], axis=1).astype(np.float32).reshape(-1, 2, 2)
    flow_trans = np.zeros((len(odom1), 2)) if odom0 is None else \
        (odom1 - np.asarray(odom0, dtype=np.float64).reshape(-1, 3))[:, :2]
    return rot, odom1[:, :2].copy(), flow_trans


def data_augmentation(sample_dict):
    """:129-144.  Host-side random left-right flip (uses the global NumPy RNG like
    the reference)."""
    scans, target_reg = sample_dict["scans"], sample_dict["target_reg"]
    if np.random.rand() < 0.5:
        scans = scans[:, ::-1]
        target_reg[:, 0] = -target_reg[:, 0]
    sample_dict.update({"target_reg": target_reg, "scans": scans})
    return sample_dict


def _phi_to_rotation_matrix(phi, is_3d=False):
    """:601-606.  Rotation about z by `phi` as a float32 matrix (2x2, or 3x3 when is_3d)."""
    c, s = np.cos(phi), np.sin(phi)
    rot = np.eye(3 if is_3d else 2, dtype=np.float32)
    rot[0, 0], rot[0, 1], rot[1, 0], rot[1, 1] = c, -s, s, c
    return rot
