"""Batched device API: torch tensors in HBM -> libpof_hip.so (C ABI) -> torch tensors.

torch is used only as the owner of device memory and streams.  Every function
validates shapes/dtypes on the host before a kernel sees them and launches on
torch's current HIP stream.  No CPU fallback exists: a missing library or a CPU
tensor raises.
"""
import collections
import ctypes as C
import functools
import inspect

import numpy as np
import torch

from . import _lib

_TAB_CACHE = {}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _aligned16(t):
    """t itself when its data starts on a 16-byte boundary, otherwise a fresh (allocator-aligned) copy."""
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def _dev(t, dtype, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError("%s must be a tensor on the HIP device (no CPU path)" % name)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return t


def phi_table(angle_inc=np.radians(0.5), num_pts=450, device="cuda"):
    """A1: device table [3N] float64 = phi | (cos, sin) interleaved.  Cached."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (float(angle_inc), int(num_pts), device.index)
    tab = _TAB_CACHE.get(key)
    if tab is None:
        tab = torch.empty(3 * num_pts, dtype=torch.float64, device=device)
        with torch.cuda.device(device):
            _lib.call("pof_laser_phi", float(angle_inc), int(num_pts), _ptr(tab), _stream())
        _TAB_CACHE[key] = tab
    return tab


def laser_phi(angle_inc=np.radians(0.5), num_pts=450, device="cuda"):
    return phi_table(angle_inc, num_pts, device)[:num_pts]


class DetCSR:
    """Ragged per-sample detections on the device: offsets [B+1] int32,
    rphi [D,2] float64, cls [D] uint8 (0 wc, 1 wa, 2 wp)."""

    def __init__(self, offsets, rphi, cls):
        self.offsets = _dev(offsets, torch.int32, "det offsets")
        self.rphi = _dev(rphi, torch.float64, "det rphi")
        self.cls = _dev(cls, torch.uint8, "det cls")
        if self.rphi.dim() != 2 or self.rphi.shape[1] != 2 or self.cls.shape[0] != self.rphi.shape[0]:
            raise ValueError("det_rphi must be [D,2] and det_cls [D]")

    @staticmethod
    def from_numpy(offsets, rphi, cls, device="cuda"):
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        if offsets[0] != 0 or np.any(np.diff(offsets) < 0) or offsets[-1] != len(rphi):
            raise ValueError("CSR offsets must start at 0, be non-decreasing and end at D")
        # keep at least one element so data_ptr() is valid for D == 0
        r = np.ascontiguousarray(rphi, dtype=np.float64).reshape(-1, 2)
        c = np.ascontiguousarray(cls, dtype=np.uint8)
        if len(r) == 0:
            r, c = np.zeros((1, 2)), np.zeros(1, dtype=np.uint8)
            d = DetCSR(torch.from_numpy(offsets).to(device), torch.from_numpy(r).to(device),
                       torch.from_numpy(c).to(device))
            return d
        return DetCSR(torch.from_numpy(offsets).to(device), torch.from_numpy(r).to(device),
                      torch.from_numpy(c).to(device))


FLOW_DISPLACEMENT, FLOW_TARGET, FLOW_VELOCITY, FLOW_PREPARED, ALIGN_NEXT_SCAN = 0, 1, 2, 3, 4


def scan_preprocess_workspace_bytes(B, D):
    return int(_lib.load().pof_scan_preprocess_workspace_bytes(int(min(B, 65535)), int(D)))


def scan_preprocess(scans, tab, odom0=None, odom1=None, dets=None, flow_kind=FLOW_DISPLACEMENT,
                    canonical=True, out_dtype=torch.float32, want=("flow",),
                    assoc_radius=(0.6, 0.4, 0.35), labels=(1, 2, 3), dyn_radius=(2.5, 2.0, 2.0),
                    out=None, workspace=None, phases=3, next_batch=None):
    """A2-A7 fused, one launch.

    scans: [B,T,N] (the last row of each window is the current scan) or [B,N].
    want: subset of {"xy","flow","closest","target_cls","target_reg","dyn_mask",
          "valid_mask","exclude_mask"}.  `out` may hold preallocated tensors.
    phases: 3 = both launches; 1 = only the per-sample params launch into
          `workspace`, 2 = only the streaming launch (for two-stream pipelining of
          independent batches; B <= 65535 in that mode).
    next_batch: chained form -- dict(odom0, odom1, dets, workspace) of the NEXT batch; this
          call then streams the current batch (its params must already be in `workspace`,
          i.e. phases is forced to 2) and evaluates the next batch's params in the same launch.
    Returns a dict of device tensors.
    """
    scans = _dev(scans, torch.float32, "scans")
    if scans.dim() == 3:
        B, T, N = scans.shape
        stride, off = T * N, (T - 1) * N
    elif scans.dim() == 2:
        B, N = scans.shape
        stride, off = N, 0
    else:
        raise ValueError("scans must be [B,T,N] or [B,N]")
    tab = _dev(tab, torch.float64, "tab")
    if tab.numel() != 3 * N:
        raise ValueError("angle table is for %d points, scans have %d" % (tab.numel() // 3, N))
    want = set(want)
    known = {"xy", "flow", "closest", "target_cls", "target_reg", "dyn_mask", "valid_mask", "exclude_mask"}
    if not want <= known:
        raise ValueError("unknown outputs: %s" % sorted(want - known))
    need_det = bool(want & {"closest", "target_cls", "target_reg", "dyn_mask", "exclude_mask"})
    if need_det and dets is None:
        raise ValueError("association / dynamic-mask outputs need detections")
    if "flow" in want:
        odom0 = _dev(odom0, torch.float64, "odom0")
        odom1 = _dev(odom1, torch.float64, "odom1")
        if tuple(odom0.shape) != (B, 3) or tuple(odom1.shape) != (B, 3):
            raise ValueError("odometry must be [B,3]")
    if dets is not None and dets.offsets.numel() != B + 1:
        raise ValueError("detection offsets must have B+1 entries")
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError("out_dtype must be float32 or float64")
    dev = scans.device
    out = {} if out is None else out

    def buf(name, shape, dtype):
        if name not in want:
            return None
        t = out.get(name)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=dev)
            out[name] = t
        else:
            _dev(t, dtype, name)
            if tuple(t.shape) != tuple(shape):
                raise ValueError("%s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
        return t

    xy = buf("xy", (B, N, 2), out_dtype)
    flow = buf("flow", (B, N, 2), out_dtype)
    closest = buf("closest", (B, N), torch.int64)
    tcls = buf("target_cls", (B, N), torch.int64)
    treg = buf("target_reg", (B, N, 2), torch.float32)
    dyn = buf("dyn_mask", (B, N), torch.float32)
    val = buf("valid_mask", (B, N), torch.float32)
    exc = buf("exclude_mask", (B, N), torch.float32)
    ar = (C.c_double * 3)(*assoc_radius)
    lb = (C.c_int32 * 3)(*labels)
    dr = (C.c_double * 3)(*dyn_radius)
    base = scans.data_ptr() + 4 * off
    D = int(dets.rphi.shape[0]) if need_det else 0
    ws_bytes = _lib.load().pof_scan_preprocess_workspace_bytes(min(B, 65535), D)
    if workspace is None:
        workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    elif workspace.numel() * workspace.element_size() < ws_bytes or not workspace.is_cuda:
        raise ValueError("workspace must be a device tensor of at least %d bytes" % ws_bytes)
    nxt = None
    if next_batch is not None:
        if B > 65535:
            raise ValueError("chained form needs B <= 65535")
        nxt = _scan_inputs(next_batch, want, flow_kind, assoc_radius, labels, dyn_radius, need_det)
    with torch.cuda.device(dev):
        # grid.y carries the sample index: chunk very large batches
        step = 65535
        for s in range(0, max(B, 1), step):
            n = min(step, B - s)
            if n <= 0:
                break

            def sl(t, per):
                return None if t is None else C.c_void_p(t.data_ptr() + s * per * t.element_size())

            _lib.call(
                "pof_scan_preprocess_chained" if nxt is not None else "pof_scan_preprocess_phase",
                C.c_void_p(base + 4 * s * stride), stride, n, N, _ptr(tab),
                sl(odom0, 3) if "flow" in want else None, sl(odom1, 3) if "flow" in want else None,
                int(flow_kind), int(bool(canonical)), int(out_dtype == torch.float64),
                sl(xy, 2 * N), sl(flow, 2 * N),
                sl(dets.offsets, 1) if need_det else None,
                _ptr(dets.rphi) if need_det else None, _ptr(dets.cls) if need_det else None, D,
                ar, lb, dr, sl(closest, N), sl(tcls, N), sl(treg, 2 * N), sl(dyn, N), sl(val, N),
                sl(exc, N), _ptr(workspace), workspace.numel() * workspace.element_size(),
                C.byref(nxt) if nxt is not None else int(phases), _stream())
    return out


_TABF = {}


def phi_table_f32(tab):
    """[N][2] float32 copy of the angle table's (cos, sin) pairs, each rounded once from its float64 entry --
    exactly what the float32-output preprocess kernel would otherwise convert per point.  Cached per table."""
    key = (tab.data_ptr(), tab.numel(), tab.device)
    t = _TABF.get(key)
    if t is None or t[0]() is not tab:
        import weakref
        n = tab.numel() // 3
        tf = tab[n:].to(torch.float32).contiguous()
        _TABF[key] = (weakref.ref(tab), tf)
        return tf
    return t[1]


def _scan_inputs(nb, want, flow_kind, assoc_radius, labels, dyn_radius, need_det):
    """pof_scan_inputs of one batch whose params are to be evaluated: dict(odom0, odom1, dets, workspace)."""
    nd = nb.get("dets")
    n0, n1 = nb.get("odom0"), nb.get("odom1")
    nws = nb["workspace"]
    nxt = _lib.ScanInputs()
    nxt.want_flow = int("flow" in want)
    if nxt.want_flow:
        n0 = _dev(n0, torch.float64, "next odom0")
        n1 = _dev(n1, torch.float64, "next odom1")
        nxt.odom0, nxt.odom1, nxt.B = n0.data_ptr(), n1.data_ptr(), n0.shape[0]
    else:
        nxt.B = nd.offsets.numel() - 1 if nd is not None else 0
    if need_det and nd is not None:
        nxt.det_offsets, nxt.det_rphi, nxt.det_cls = nd.offsets.data_ptr(), nd.rphi.data_ptr(), nd.cls.data_ptr()
        nxt.D = int(nd.rphi.shape[0])
    nxt.flow_kind = int(flow_kind)
    nxt.assoc_radius = (C.c_double * 3)(*assoc_radius)
    nxt.labels = (C.c_int32 * 3)(*labels)
    nxt.dyn_radius = (C.c_double * 3)(*dyn_radius)
    nxt.workspace = nws.data_ptr()
    nxt.workspace_bytes = nws.numel() * nws.element_size()
    return nxt


SCAN_MAX_SLOTS = _lib.SCAN_MAX_SLOTS     # batches one launch of scan_preprocess_multi may stream (and evaluate params for)


def scan_preprocess_multi(batches, tab, next_batches=(), flow_kind=FLOW_DISPLACEMENT, canonical=True,
                          out_dtype=torch.float32, want=("flow",), assoc_radius=(0.6, 0.4, 0.35), labels=(1, 2, 3),
                          dyn_radius=(2.5, 2.0, 2.0), prepare=False):
    """A2-A7 fused for up to SCAN_MAX_SLOTS (8) batches in ONE launch (pof_scan_preprocess_multi): a loader that runs ahead hands
    over several ring slots at once.

    batches: list of dict(scans [B,T,N] | [B,N], dets (DetCSR or None), out {name: tensor}, workspace) -- the
             workspaces must already hold the batches' params (an earlier call's `next_batches`); every name in
             `want` must be preallocated in `out`.
    next_batches: list of dict(odom0, odom1, dets, workspace) whose params this launch evaluates on extra
             workgroups.  `batches` may be empty (params only: priming the ring).
    prepare: do not launch; return a PreparedScanLaunch that does (the arguments marshalled once).
    """
    want = set(want)
    known = {"xy", "flow", "closest", "target_cls", "target_reg", "dyn_mask", "valid_mask", "exclude_mask"}
    if not want <= known:
        raise ValueError("unknown outputs: %s" % sorted(want - known))
    if len(batches) > _lib.SCAN_MAX_SLOTS or len(next_batches) > _lib.SCAN_MAX_SLOTS:
        raise ValueError("at most %d batches per launch" % _lib.SCAN_MAX_SLOTS)
    need_det = bool(want & {"closest", "target_cls", "target_reg", "dyn_mask", "exclude_mask"})
    tab = _dev(tab, torch.float64, "tab")
    N = tab.numel() // 3
    cur = (_lib.ScanBatch * max(len(batches), 1))()
    keep = []
    for k, bt in enumerate(batches):
        scans = _dev(bt["scans"], torch.float32, "scans")
        if scans.dim() == 3:
            B, T, n = scans.shape
            stride, off = T * n, (T - 1) * n
        elif scans.dim() == 2:
            B, n = scans.shape
            stride, off = n, 0
        else:
            raise ValueError("scans must be [B,T,N] or [B,N]")
        if n != N:
            raise ValueError("angle table is for %d points, scans have %d" % (N, n))
        dets = bt.get("dets")
        if need_det and dets is None:
            raise ValueError("association / dynamic-mask outputs need detections")
        if dets is not None and dets.offsets.numel() != B + 1:
            raise ValueError("detection offsets must have B+1 entries")
        out, ws = bt["out"], bt["workspace"]
        c = cur[k]
        c.ranges, c.sample_stride, c.B = scans.data_ptr() + 4 * off, stride, B
        c.D = int(dets.rphi.shape[0]) if need_det else 0
        c.det_offsets = dets.offsets.data_ptr() if need_det else None
        shapes = {"xy": ((B, N, 2), out_dtype), "flow": ((B, N, 2), out_dtype), "closest": ((B, N), torch.int64),
                  "target_cls": ((B, N), torch.int64), "target_reg": ((B, N, 2), torch.float32),
                  "dyn_mask": ((B, N), torch.float32), "valid_mask": ((B, N), torch.float32),
                  "exclude_mask": ((B, N), torch.float32)}
        if (scans.data_ptr() + 4 * off) % 8 or stride % 2:
            raise ValueError("batch %d: the current scans must start on an 8-byte boundary with an even sample stride"
                             % k)
        for name in known:
            if name in want:
                t = _dev(out[name], shapes[name][1], name)
                if tuple(t.shape) != shapes[name][0]:
                    raise ValueError("%s has shape %s, expected %s" % (name, tuple(t.shape), shapes[name][0]))
                if t.data_ptr() % 16:
                    raise ValueError("batch %d: output %s must start on a 16-byte boundary (the one-launch form "
                                     "has no unaligned variant; use scan_preprocess)" % (k, name))
                setattr(c, name, t.data_ptr())
        c.workspace, c.workspace_bytes = ws.data_ptr(), ws.numel() * ws.element_size()
        keep.append((scans, out, ws))
    nxt = (_lib.ScanInputs * max(len(next_batches), 1))()
    for k, nb in enumerate(next_batches):
        nxt[k] = _scan_inputs(nb, want, flow_kind, assoc_radius, labels, dyn_radius, need_det)
    tabf = phi_table_f32(tab) if out_dtype == torch.float32 else None
    args = (cur, len(batches), nxt, len(next_batches), N, _ptr(tab), _ptr(tabf), int(flow_kind), int(bool(canonical)),
            int(out_dtype == torch.float64), (C.c_double * 3)(*assoc_radius), (C.c_int32 * 3)(*labels),
            (C.c_double * 3)(*dyn_radius))
    if prepare:
        return PreparedScanLaunch(args, tab.device, (keep, list(next_batches), tab, tabf))
    with torch.cuda.device(tab.device):
        _lib.call("pof_scan_preprocess_multi", *args, _stream())


class PreparedScanLaunch:
    """A marshalled pof_scan_preprocess_multi call (``scan_preprocess_multi(..., prepare=True)``): a loader that cycles
    through a ring of fixed buffers builds the descriptor tables of its (current slots, next slots) combinations once
    and then pays one ctypes call per launch -- a few microseconds of host time instead of the ~100 us the checked,
    per-call marshalling of 8 + 8 batches costs.  The tensors it points at are kept alive by the object."""

    def __init__(self, args, device, keep):
        self._args, self._device, self._keep = args, device, keep
        self._fn = getattr(_lib.load(), "pof_scan_preprocess_multi")

    def __call__(self):
        code = self._fn(*self._args, torch.cuda.current_stream(self._device).cuda_stream)
        if code != _lib.POF_OK:
            _lib.raise_for("pof_scan_preprocess_multi", code)


def flow_from_xy(xy, odom0, odom1, flow_kind=FLOW_DISPLACEMENT, canonical=False, tab=None):
    """A3 on scanner-frame points: xy [B,N,2] float64, odom [B,3] float64 -> flow [B,N,2] float64."""
    xy = _dev(xy, torch.float64, "xy")
    odom0 = _dev(odom0, torch.float64, "odom0")
    odom1 = _dev(odom1, torch.float64, "odom1")
    if xy.dim() != 3 or xy.shape[-1] != 2 or tuple(odom0.shape) != (xy.shape[0], 3) or odom0.shape != odom1.shape:
        raise ValueError("xy must be [B,N,2] and odometry [B,3]")
    if canonical and (tab is None or tab.numel() != 3 * xy.shape[1]):
        raise ValueError("canonical output needs the angle table of this N")
    out = torch.empty_like(xy)
    with torch.cuda.device(xy.device):
        _lib.call("pof_flow_from_xy", _ptr(xy), _ptr(odom0), _ptr(odom1), int(flow_kind), int(bool(canonical)),
                  _ptr(tab), _ptr(out), xy.shape[0], xy.shape[1], _stream())
    return out


def xy_to_rphi(x, y):
    """A2 inverse on float64 device tensors of equal shape."""
    x = _dev(x, torch.float64, "x")
    y = _dev(y, torch.float64, "y")
    if x.shape != y.shape:
        raise ValueError("x and y must have the same shape")
    r, phi = torch.empty_like(x), torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.call("pof_xy_to_rphi", _ptr(x), _ptr(y), _ptr(r), _ptr(phi), x.numel(), _stream())
    return r, phi


def rotate_flow(flow, tab, to_canonical=True, out=None):
    """A4 on a [B,N,2] (or [N,2]) float32/float64 device tensor."""
    if flow.dtype not in (torch.float32, torch.float64):
        raise TypeError("flow must be float32 or float64")
    flow = _dev(flow, flow.dtype, "flow")
    N = flow.shape[-2]
    B = flow.numel() // (2 * N)
    if flow.shape[-1] != 2 or tab.numel() != 3 * N:
        raise ValueError("flow must be [...,N,2] matching the angle table")
    out = torch.empty_like(flow) if out is None else out
    with torch.cuda.device(flow.device):
        _lib.call("pof_rotate_flow", _ptr(flow), _ptr(out), _ptr(tab), B, N, int(bool(to_canonical)),
                  int(flow.dtype == torch.float64), _stream())
    return out


def det_to_canonical(ranges, tab, det_r, det_phi):
    """A5 forward, batched per point: ranges [B,N] float32, det_* [B,N] float64."""
    ranges = _dev(ranges, torch.float32, "ranges")
    B, N = ranges.shape
    det_r = _dev(det_r, torch.float64, "det_r")
    det_phi = _dev(det_phi, torch.float64, "det_phi")
    dx, dy = torch.empty_like(det_r), torch.empty_like(det_r)
    with torch.cuda.device(ranges.device):
        _lib.call("pof_det_to_canonical", _ptr(ranges), _ptr(tab), _ptr(det_r), _ptr(det_phi), _ptr(dx),
                  _ptr(dy), B, N, _stream())
    return dx, dy


def canonical_to_det(ranges, tab, dx, dy):
    """A5 inverse."""
    ranges = _dev(ranges, torch.float32, "ranges")
    B, N = ranges.shape
    dx = _dev(dx, torch.float64, "dx")
    dy = _dev(dy, torch.float64, "dy")
    r, p = torch.empty_like(dx), torch.empty_like(dx)
    with torch.cuda.device(ranges.device):
        _lib.call("pof_canonical_to_det", _ptr(ranges), _ptr(tab), _ptr(dx), _ptr(dy), _ptr(r), _ptr(p),
                  B, N, _stream())
    return r, p


def cutout(scans, tab, stride=1, centered=True, fixed=False, window_width=1.66, window_depth=1.0,
           num_cutout_pts=48, padding_val=29.99, area_mode=False, out=None, return_debug=False,
           exact_values=True, out_dtype=torch.float32, workspace=None):
    """A8 for a batch: scans [B,T,N] float32 -> [B, ceil(N/stride), T, P] float32.
    exact_values=False selects the float32 value path (exact indices, values within 1e-5; samples that meet a
    range of 64 m or more are computed with the exact path's float64 sequence);
    out_dtype=torch.float16 stores the result as float16 (BASELINE config 5).
    workspace: optional caller-owned int32 tensor of >= min(B, 65535) elements (the per-sample area maxima); a
    caller that captures this call in a hipGraph passes one it allocated BEFORE the capture, so that the graph
    holds no allocation of its own for it (streaming.StreamingDetector)."""
    if out_dtype not in (torch.float32, torch.float16):
        raise TypeError("out_dtype must be float32 or float16")
    scans = _dev(scans, torch.float32, "scans")
    if scans.dim() != 3:
        raise ValueError("scans must be [B,T,N]")
    B, T, N = scans.shape
    if tab.numel() != 3 * N:
        raise ValueError("angle table does not match N")
    Ns = (N + stride - 1) // stride
    P = int(num_cutout_pts)
    if out is None:
        out = torch.empty((B, Ns, T, P), dtype=out_dtype, device=scans.device)
    else:
        _dev(out, out_dtype, "out")
        if tuple(out.shape) != (B, Ns, T, P):
            raise ValueError("out has the wrong shape")
    entry = "pof_cutout_ex" if out_dtype == torch.float32 else "pof_cutout_f16"
    dbg = torch.empty((B, P, T, Ns), dtype=torch.int32, device=scans.device) if return_debug else None
    dbg_area = None
    with torch.cuda.device(scans.device):
        step = 65535
        for s in range(0, B, step):
            n = min(step, B - s)
            if workspace is not None:
                ws = _dev(workspace, torch.int32, "workspace")
                if ws.numel() < n:
                    raise ValueError("workspace must hold at least %d int32 elements" % n)
            else:
                ws = torch.empty(max(n, 1), dtype=torch.int32, device=scans.device)
            _lib.call(entry, _ptr(scans[s:s + n]), n, T, N, _ptr(tab), int(stride), int(bool(centered)),
                      int(bool(fixed)), float(window_width), float(window_depth), P, float(padding_val),
                      int(bool(area_mode)), 0 if exact_values else 1, _ptr(out[s:s + n]), _ptr(ws),
                      _ptr(dbg[s:s + n]) if dbg is not None else None, _stream())
            if return_debug:
                dbg_area = ws
    if return_debug:
        return out, {"lo": dbg, "s_area": dbg_area}
    return out


def conv3_bn_lrelu(x, wt, scale, shift, pool=False, negative_slope=0.1, out=None):
    """N2 trunk layer (inference): x [S,Ci,L] f32, wt [3,Ci,Co] f32 (conv weight transposed), scale/shift [Co]
    (folded BatchNorm + bias) -> [S, Co, L//2 if pool else L].  x in float16 storage (BASELINE config 5): out is
    float16 as well -- the float32 layer on the same values, rounded once."""
    half = isinstance(x, torch.Tensor) and x.dtype == torch.float16
    act = torch.float16 if half else torch.float32
    x = _dev(x, act, "x")
    wt = _dev(wt, torch.float32, "wt")
    scale = _dev(scale, torch.float32, "scale")
    shift = _dev(shift, torch.float32, "shift")
    S, Ci, L = x.shape
    if wt.dim() != 3 or wt.shape[0] != 3 or wt.shape[1] != Ci:
        raise ValueError("wt must be [3, Ci, Co]")
    Co = wt.shape[2]
    if scale.numel() != Co or shift.numel() != Co:
        raise ValueError("scale / shift must have Co entries")
    Lout = L // 2 if pool else L
    if out is None:
        out = torch.empty((S, Co, Lout), dtype=act, device=x.device)
    else:
        _dev(out, act, "out")
    if S > 0:
        with torch.cuda.device(x.device):
            _lib.call("pof_conv3_bn_lrelu_f16" if half else "pof_conv3_bn_lrelu", _ptr(x), _ptr(wt), _ptr(scale), _ptr(shift), S, Ci, Co, L,
                      int(bool(pool)), float(negative_slope), _ptr(out), _stream())
    return out


def conv3_first_two(x, l1, wt, scale, shift, slope1=0.1, pool=False, negative_slope=0.1, out=None):
    """The trunk's first two units in one launch (inference): x [S,L] or [S,1,L] f32 (single-channel cutouts), l1 [C1,4]
    f32 = the first unit as {a0, a1, a2, b} per channel (taps x folded BatchNorm scale, shift), wt [3,C1,Co] /
    scale / shift [Co] = the second unit -> [S, Co, L//2 if pool else L].  A float16 cutout (cutout(out_dtype=float16))
    gives a float16 out: the float32 call on the same values, rounded once."""
    half = isinstance(x, torch.Tensor) and x.dtype == torch.float16
    act = torch.float16 if half else torch.float32
    x = _dev(x, act, "x")
    if x.dim() == 3 and x.shape[1] == 1:
        x = x.view(x.shape[0], x.shape[2])
    if x.dim() != 2:
        raise ValueError("x must be [S, L] or [S, 1, L]")
    l1 = _dev(l1, torch.float32, "l1")
    wt = _dev(wt, torch.float32, "wt")
    scale = _dev(scale, torch.float32, "scale")
    shift = _dev(shift, torch.float32, "shift")
    S, L = x.shape
    if l1.dim() != 2 or l1.shape[1] != 4 or l1.shape[0] > 128:
        raise ValueError("l1 must be [C1 <= 128, 4]")
    C1 = l1.shape[0]
    if wt.dim() != 3 or wt.shape[0] != 3 or wt.shape[1] != C1:
        raise ValueError("wt must be [3, C1, Co]")
    Co = wt.shape[2]
    if scale.numel() != Co or shift.numel() != Co:
        raise ValueError("scale / shift must have Co entries")
    if pool and L % 2:
        raise ValueError("pooled output needs an even L")
    if out is None:
        out = torch.empty((S, Co, L // 2 if pool else L), dtype=act, device=x.device)
    else:
        _dev(out, act, "out")
    if S > 0:
        with torch.cuda.device(x.device):
            _lib.call("pof_conv3_first_two_f16" if half else "pof_conv3_first_two", _ptr(x), _ptr(l1), float(slope1), _ptr(wt), _ptr(scale), _ptr(shift), S, C1, Co,
                      L, int(bool(pool)), float(negative_slope), _ptr(out), _stream())
    return out


def conv1d_bn_lrelu(x, wt, scale, shift, stride=1, pool=False, negative_slope=0.1, out=None):
    """Conv1d(kernel 1 | 3, padding kernel // 2, stride 1 | 2) + folded BatchNorm + LeakyReLU [+ max_pool1d(2)] on the
    float32-MFMA implicit-GEMM kernel: x [S,Ci,L] f32, wt [kernel,Ci,Co] f32 (conv weight transposed), scale / shift
    [Co] -> [S, Co, Lc] with Lc = L (stride 1) | (L + 1) // 2 (stride 2), halved when pooled."""
    x = _dev(x, torch.float32, "x")
    wt = _dev(wt, torch.float32, "wt")
    scale = _dev(scale, torch.float32, "scale")
    shift = _dev(shift, torch.float32, "shift")
    S, Ci, L = x.shape
    if wt.dim() != 3 or wt.shape[0] not in (1, 3) or wt.shape[1] != Ci:
        raise ValueError("wt must be [1 | 3, Ci, Co]")
    K, Co = int(wt.shape[0]), int(wt.shape[2])
    if scale.numel() != Co or shift.numel() != Co:
        raise ValueError("scale / shift must have Co entries")
    Lc = L if stride == 1 else (L + 1) // 2
    Lout = Lc // 2 if pool else Lc
    if out is None:
        out = torch.empty((S, Co, Lout), dtype=torch.float32, device=x.device)
    else:
        _dev(out, torch.float32, "out")
    if S > 0:
        with torch.cuda.device(x.device):
            _lib.call("pof_conv1d_bn_lrelu", _ptr(x), _ptr(wt), _ptr(scale), _ptr(shift), S, Ci, Co, L, K, int(stride),
                      int(bool(pool)), float(negative_slope), _ptr(out), _stream())
    return out


def conv1d_plan(S, Ci, Co, L, kernel_size=3, stride=1, pool=False, fused_first=False):
    """Host-only: the kernel form conv3_bn_lrelu / conv1d_bn_lrelu / conv3_first_two (``fused_first``, Ci = C1) would
    launch for these sizes -> dict(split_k, channels_per_workgroup, launches, wide_offsets); the first two describe the
    first launch.  No device work."""
    out = [C.c_int(0) for _ in range(4)]
    _lib.call("pof_conv1d_plan", int(S), int(Ci), int(Co), int(L), int(kernel_size), int(stride), int(bool(pool)),
              int(bool(fused_first)), *[C.byref(v) for v in out])
    return dict(split_k=bool(out[0].value), channels_per_workgroup=out[1].value, launches=out[2].value,
                wide_offsets=out[3].value)


def drow_heads(feat, w_cls, b_cls, w_reg, b_reg):
    """N2 heads (inference): feat [S,C,L] f32, w_cls [n_cls,C], w_reg [2,C] -> (pred_cls [S,n_cls], pred_reg [S,2]):
    mean over positions + both 1x1 convolutions in one launch.  feat may be in float16 storage; outputs are float32."""
    half = isinstance(feat, torch.Tensor) and feat.dtype == torch.float16
    feat = _dev(feat, torch.float16 if half else torch.float32, "feat")
    S, C, L = feat.shape
    w_cls = _dev(w_cls.reshape(-1, C), torch.float32, "w_cls")
    w_reg = _dev(w_reg.reshape(-1, C), torch.float32, "w_reg")
    b_cls, b_reg = _dev(b_cls, torch.float32, "b_cls"), _dev(b_reg, torch.float32, "b_reg")
    n_cls = w_cls.shape[0]
    if w_reg.shape[0] != 2 or b_cls.numel() != n_cls or b_reg.numel() != 2:
        raise ValueError("heads: w_cls [n_cls, C], b_cls [n_cls], w_reg [2, C], b_reg [2]")
    pred_cls = torch.empty((S, n_cls), dtype=torch.float32, device=feat.device)
    pred_reg = torch.empty((S, 2), dtype=torch.float32, device=feat.device)
    if S > 0:
        with torch.cuda.device(feat.device):
            _lib.call("pof_drow_heads_f16" if half else "pof_drow_heads", _ptr(feat), S, C, L, _ptr(w_cls), _ptr(b_cls), n_cls, _ptr(w_reg), _ptr(b_reg),
                      _ptr(pred_cls), _ptr(pred_reg), _stream())
    return pred_cls, pred_reg


def conv3_wgrad_supported(S, Ci, Co, L, kernel_size=3):
    return S > 0 and int(_lib.load().pof_conv1d_wgrad_workspace_bytes(int(S), int(Ci), int(Co), int(L),
                                                                      int(kernel_size))) > 0


def conv3_wgrad(x, dy, kernel_size=3):
    """N2 training: weight gradient of Conv1d(k = 3 | 1, pad = k // 2): x [S,Ci,L] f32, dy [S,Co,L] f32 ->
    dw [Co,Ci,k] f32."""
    x = _dev(x, torch.float32, "x")
    dy = _dev(dy, torch.float32, "dy")
    S, Ci, L = x.shape
    if dy.dim() != 3 or dy.shape[0] != S or dy.shape[2] != L:
        raise ValueError("dy must be [S, Co, L]")
    if kernel_size not in (1, 3):
        raise ValueError("kernel_size must be 1 or 3")
    Co = dy.shape[1]
    # the library picks its load width from the operands' alignment and sizes the workspace (and the shapes it takes)
    # for 16-byte aligned ones: a view at an offset goes through an aligned copy
    x = _aligned16(x)
    dy = _aligned16(dy)
    nbytes = int(_lib.load().pof_conv1d_wgrad_workspace_bytes(S, Ci, Co, L, kernel_size))
    if nbytes == 0:
        raise ValueError("conv3_wgrad: unsupported shape S=%d Ci=%d Co=%d L=%d" % (S, Ci, Co, L))
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=x.device)
    dw = torch.empty((Co, Ci, kernel_size), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.call("pof_conv1d_wgrad", _ptr(x), _ptr(dy), S, Ci, Co, L, kernel_size, _ptr(dw), _ptr(ws), nbytes,
                  _stream())
    return dw


def regression_loss2(pred, target, alpha=0.5, with_grad=True):
    """configs[3] loss: pred, target [B,3|5] f32 -> (loss [] f32, d loss / d pred [B,T] f32 or None) in one launch."""
    pred = _dev(pred, torch.float32, "pred")
    target = _dev(target, torch.float32, "target")
    if pred.dim() != 2 or tuple(target.shape) != tuple(pred.shape) or pred.shape[1] not in (3, 5) or pred.shape[0] < 1:
        raise ValueError("pred and target must be [B, 3] or [B, 5] with B >= 1")
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    dpred = torch.empty_like(pred) if with_grad else None
    with torch.cuda.device(pred.device):
        _lib.call("pof_regression_loss2", _ptr(pred), _ptr(target), pred.shape[0], pred.shape[1], float(alpha), _ptr(loss),
                  _ptr(dpred), _stream())
    return loss, dpred


def linear_bias(x, weight, bias=None, out=None):
    """configs[3] dense layers: x [B,K] f32, weight [N,K] f32 (torch.nn.Linear's), bias [N] f32 or None -> x @ weight.T
    + bias [B,N] on the small-batch MFMA kernel (K a multiple of 4)."""
    x = _dev(x, torch.float32, "x")
    weight = _dev(weight, torch.float32, "weight")
    if x.dim() != 2 or weight.dim() != 2 or weight.shape[1] != x.shape[1]:
        raise ValueError("x must be [B, K] and weight [N, K]")
    B, K = x.shape
    N = weight.shape[0]
    if K % 4:
        raise ValueError("linear_bias: K = %d is not a multiple of 4" % K)
    x = _aligned16(x)                # 16-byte operand loads: views at an offset go through a copy
    weight = _aligned16(weight)
    if bias is not None and _dev(bias, torch.float32, "bias").numel() != N:
        raise ValueError("bias must have N entries")
    if out is None:
        out = torch.empty((B, N), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (B, N) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
        raise ValueError("out must be a contiguous float32 [B, N] tensor on x's device")
    if B == 0:
        return out
    with torch.cuda.device(x.device):
        _lib.call("pof_linear_bias", _ptr(x), _ptr(weight), _ptr(bias), B, K, N, _ptr(out), _stream())
    return out


def bn_lrelu_pool_supported(S, C, L, pool=False, groups=1):
    """True when the fused training tail covers this shape (L <= 256, C*L % 4 == 0, S % groups == 0; pool = True / 1:
    max over pairs, L even; pool = 2: max over the whole row, L a power of two >= 4)."""
    if int(pool) == 1 and (L & 1):
        return False
    if int(pool) == 2 and (L < 4 or L & (L - 1)):
        return False
    return S > 0 and int(_lib.load().pof_bn_lrelu_pool_workspace_bytes(int(S), int(C), int(L), int(groups))) > 0


def _bn_workspace(S, C, L, groups, device):
    nbytes = int(_lib.load().pof_bn_lrelu_pool_workspace_bytes(int(S), int(C), int(L), int(groups)))
    if nbytes == 0:
        raise ValueError("bn_lrelu_pool: unsupported shape S=%d C=%d L=%d groups=%d (needs L <= 256, C*L %% 4 == 0, "
                         "S %% groups == 0)" % (S, C, L, groups))
    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device), nbytes


def bn_lrelu_pool_forward(y, gamma, beta, running_mean=None, running_var=None, momentum=0.1, eps=1e-5,
                          negative_slope=0.1, pool=False, groups=1):
    """N2 training tail: y [S,C,L] f32 (convolution output) -> (z [S,C,L or L//2], save_mean [groups*C],
    save_invstd [groups*C]); z = max_pool1d?(leaky_relu(batch_norm_train(y))), the batch statistics taken separately
    over each of `groups` equal contiguous ranges of the sequences.  running_mean / running_var are updated in
    place (once per group, in order).  pool = 2: the maximum over the whole row, z [S,C] (the PointNet's max over
    points)."""
    y = _dev(y, torch.float32, "y")
    gamma = _dev(gamma, torch.float32, "gamma")
    beta = _dev(beta, torch.float32, "beta")
    S, C, L = y.shape
    if gamma.numel() != C or beta.numel() != C:
        raise ValueError("gamma / beta must have C entries")
    for name, t in (("running_mean", running_mean), ("running_var", running_var)):
        if t is not None and (_dev(t, torch.float32, name).numel() != C):
            raise ValueError("%s must have C entries" % name)
    ws, nbytes = _bn_workspace(S, C, L, groups, y.device)
    pool = int(pool)
    if not bn_lrelu_pool_supported(S, C, L, pool, groups):
        raise ValueError("bn_lrelu_pool: pool mode %d does not take L = %d" % (pool, L))
    out = torch.empty((S, C) if pool == 2 else (S, C, L // 2 if pool else L), dtype=torch.float32, device=y.device)
    mean = torch.empty(groups * C, dtype=torch.float32, device=y.device)
    invstd = torch.empty(groups * C, dtype=torch.float32, device=y.device)
    with torch.cuda.device(y.device):
        _lib.call("pof_bn_lrelu_pool_forward", _ptr(y), S, C, L, int(groups), _ptr(gamma), _ptr(beta),
                  _ptr(running_mean), _ptr(running_var), float(momentum), float(eps), float(negative_slope),
                  pool, _ptr(out), _ptr(mean), _ptr(invstd), _ptr(ws), nbytes, _stream())
    return out, mean, invstd


def bn_lrelu_pool_backward(y, dz, gamma, beta, save_mean, save_invstd, negative_slope=0.1, pool=False,
                           bias_grad=False, groups=1):
    """Backward of bn_lrelu_pool_forward: -> (dy [S,C,L], dgamma [C], dbeta [C]) and, with ``bias_grad``, also
    sum(dy) over (S, L) [C] -- the gradient of the convolution bias in front of the BatchNorm."""
    y = _dev(y, torch.float32, "y")
    dz = _dev(dz, torch.float32, "dz")
    S, C, L = y.shape
    pool = int(pool)
    if not bn_lrelu_pool_supported(S, C, L, pool, groups):
        raise ValueError("bn_lrelu_pool: pool mode %d does not take L = %d" % (pool, L))
    if tuple(dz.shape) != ((S, C) if pool == 2 else (S, C, L // 2 if pool else L)):
        raise ValueError("dz must be [S, C%s]" % ("" if pool == 2 else ", L//2" if pool else ", L"))
    for name, t, n in (("gamma", gamma, C), ("beta", beta, C), ("save_mean", save_mean, groups * C),
                       ("save_invstd", save_invstd, groups * C)):
        if _dev(t, torch.float32, name).numel() != n:
            raise ValueError("%s must have %d entries" % (name, n))
    ws, nbytes = _bn_workspace(S, C, L, groups, y.device)
    dy = torch.empty_like(y)
    dgamma = torch.empty(C, dtype=torch.float32, device=y.device)
    dbeta = torch.empty(C, dtype=torch.float32, device=y.device)
    dbias = torch.empty(C, dtype=torch.float32, device=y.device) if bias_grad else None
    with torch.cuda.device(y.device):
        _lib.call("pof_bn_lrelu_pool_backward", _ptr(y), _ptr(dz), S, C, L, int(groups), _ptr(gamma), _ptr(beta),
                  _ptr(save_mean), _ptr(save_invstd), float(negative_slope), pool, _ptr(dy), _ptr(dgamma),
                  _ptr(dbeta), _ptr(dbias), _ptr(ws), nbytes, _stream())
    return (dy, dgamma, dbeta, dbias) if bias_grad else (dy, dgamma, dbeta)


def _bn_sync_shape(y, pool, groups):
    y = _dev(y, torch.float32, "y")
    S, C, L = y.shape
    pool = int(pool)
    if not bn_lrelu_pool_supported(S, C, L, pool, groups):
        raise ValueError("bn_sync: unsupported shape S=%d C=%d L=%d groups=%d pool mode %d" % (S, C, L, groups, pool))
    return y, S, C, L, pool


def bn_sync_forward_stats(y, groups=1):
    """First half of the global-batch tail: y [S,C,L] f32 -> stat [groups*(2C+1)] f64, per group
    sum y [C] | sum y^2 [C] | count.  The ranks add their ``stat`` (one all-reduce) before bn_sync_forward_apply."""
    y, S, C, L, _ = _bn_sync_shape(y, 0, groups)
    ws, nbytes = _bn_workspace(S, C, L, groups, y.device)
    stat = torch.empty(groups * (2 * C + 1), dtype=torch.float64, device=y.device)
    with torch.cuda.device(y.device):
        _lib.call("pof_bn_sync_forward_stats", _ptr(y), S, C, L, int(groups), _ptr(stat), _ptr(ws), nbytes, _stream())
    return stat


def bn_sync_forward_apply(y, stat, gamma, beta, running_mean=None, running_var=None, momentum=0.1, eps=1e-5,
                          negative_slope=0.1, pool=False, groups=1):
    """Second half: the summed ``stat`` -> (z, save_mean [groups*C], save_invstd [groups*C]) as bn_lrelu_pool_forward
    gives them, the statistics being those of the global batch; the running statistics are updated in place with the
    unbiased variance over the global count."""
    y, S, C, L, pool = _bn_sync_shape(y, pool, groups)
    gamma = _dev(gamma, torch.float32, "gamma")
    beta = _dev(beta, torch.float32, "beta")
    if gamma.numel() != C or beta.numel() != C:
        raise ValueError("gamma / beta must have C entries")
    if _dev(stat, torch.float64, "stat").numel() != groups * (2 * C + 1):
        raise ValueError("stat must have groups * (2C + 1) entries")
    for name, t in (("running_mean", running_mean), ("running_var", running_var)):
        if t is not None and (_dev(t, torch.float32, name).numel() != C):
            raise ValueError("%s must have C entries" % name)
    ws, nbytes = _bn_workspace(S, C, L, groups, y.device)
    out = torch.empty((S, C) if pool == 2 else (S, C, L // 2 if pool else L), dtype=torch.float32, device=y.device)
    mean = torch.empty(groups * C, dtype=torch.float32, device=y.device)
    invstd = torch.empty(groups * C, dtype=torch.float32, device=y.device)
    with torch.cuda.device(y.device):
        _lib.call("pof_bn_sync_forward_apply", _ptr(y), S, C, L, int(groups), _ptr(stat), _ptr(gamma), _ptr(beta),
                  _ptr(running_mean), _ptr(running_var), float(momentum), float(eps), float(negative_slope), pool,
                  _ptr(out), _ptr(mean), _ptr(invstd), _ptr(ws), nbytes, _stream())
    return out, mean, invstd


def _bn_sync_backward_args(y, dz, gamma, beta, save_mean, save_invstd, pool, groups):
    y, S, C, L, pool = _bn_sync_shape(y, pool, groups)
    dz = _dev(dz, torch.float32, "dz")
    if tuple(dz.shape) != ((S, C) if pool == 2 else (S, C, L // 2 if pool else L)):
        raise ValueError("dz must be [S, C%s]" % ("" if pool == 2 else ", L//2" if pool else ", L"))
    for name, t, n in (("gamma", gamma, C), ("beta", beta, C), ("save_mean", save_mean, groups * C),
                       ("save_invstd", save_invstd, groups * C)):
        if _dev(t, torch.float32, name).numel() != n:
            raise ValueError("%s must have %d entries" % (name, n))
    return y, dz, S, C, L, pool


def bn_sync_backward_reduce(y, dz, gamma, beta, save_mean, save_invstd, negative_slope=0.1, pool=False, groups=1):
    """First half of the backward pass: -> (red [groups*2C] f64 = per group sum dU [C] | sum dU*xhat [C], undivided;
    dgamma [C], dbeta [C] of this rank's samples).  The ranks add their ``red`` before bn_sync_backward_apply."""
    y, dz, S, C, L, pool = _bn_sync_backward_args(y, dz, gamma, beta, save_mean, save_invstd, pool, groups)
    ws, nbytes = _bn_workspace(S, C, L, groups, y.device)
    red = torch.empty(groups * 2 * C, dtype=torch.float64, device=y.device)
    dgamma = torch.empty(C, dtype=torch.float32, device=y.device)
    dbeta = torch.empty(C, dtype=torch.float32, device=y.device)
    with torch.cuda.device(y.device):
        _lib.call("pof_bn_sync_backward_reduce", _ptr(y), _ptr(dz), S, C, L, int(groups), _ptr(gamma), _ptr(beta),
                  _ptr(save_mean), _ptr(save_invstd), float(negative_slope), pool, _ptr(red), _ptr(dgamma),
                  _ptr(dbeta), _ptr(ws), nbytes, _stream())
    return red, dgamma, dbeta


def bn_sync_backward_apply(y, dz, gamma, beta, save_mean, save_invstd, red, stat, negative_slope=0.1, pool=False,
                           bias_grad=False, groups=1):
    """Second half: the summed ``red`` and the forward's summed ``stat`` (for the global count) -> dy [S,C,L] and, with
    ``bias_grad``, (dy, sum(dy) over (S, L) [C])."""
    y, dz, S, C, L, pool = _bn_sync_backward_args(y, dz, gamma, beta, save_mean, save_invstd, pool, groups)
    if _dev(red, torch.float64, "red").numel() != groups * 2 * C:
        raise ValueError("red must have groups * 2C entries")
    if _dev(stat, torch.float64, "stat").numel() != groups * (2 * C + 1):
        raise ValueError("stat must have groups * (2C + 1) entries")
    ws, nbytes = _bn_workspace(S, C, L, groups, y.device)
    dy = torch.empty_like(y)
    dbias = torch.empty(C, dtype=torch.float32, device=y.device) if bias_grad else None
    with torch.cuda.device(y.device):
        _lib.call("pof_bn_sync_backward_apply", _ptr(y), _ptr(dz), S, C, L, int(groups), _ptr(gamma), _ptr(beta),
                  _ptr(save_mean), _ptr(save_invstd), _ptr(red), _ptr(stat), float(negative_slope), pool, _ptr(dy),
                  _ptr(dbias), _ptr(ws), nbytes, _stream())
    return (dy, dbias) if bias_grad else dy


def segment_inputs(points, centers, oris, radius=0.4, input_size=64, min_segment_size=5, seed=0,
                   return_mask=False):
    """N3: points [Np,D] f64, centers [S,D] f64, oris [S] f64 -> (x [S,input_size,D+1] f32, count [S] i32
    [, mask [S,Np] bool]): radius query + fixed-size resampling of every detection's segment in one launch."""
    points = _dev(points, torch.float64, "points")
    centers = _dev(centers, torch.float64, "centers")
    oris = _dev(oris, torch.float64, "oris")
    if points.dim() != 2 or centers.dim() != 2 or points.shape[1] != centers.shape[1]:
        raise ValueError("points [Np,D] and centers [S,D] must share D")
    Np, D = points.shape
    S = centers.shape[0]
    if oris.numel() != S:
        raise ValueError("one orientation per detection")
    dev = points.device
    x = torch.zeros((S, int(input_size), D + 1), dtype=torch.float32, device=dev)
    count = torch.zeros((S,), dtype=torch.int32, device=dev)
    mask = torch.zeros((S, Np), dtype=torch.uint8, device=dev) if return_mask else None
    if S > 0 and Np > 0:
        with torch.cuda.device(dev):
            _lib.call("pof_segment_inputs", _ptr(points), Np, D, _ptr(centers), _ptr(oris), S, float(radius),
                      int(input_size), int(min_segment_size), int(seed) & 0xFFFFFFFF, _ptr(x), _ptr(count),
                      _ptr(mask) if mask is not None else None, _stream())
    if return_mask:
        return x, count, mask.bool()
    return x, count


def segment_resample(points, seg_offsets, centers, extra=None, random_drop=0.0, input_size=64, seed=0,
                     max_segment=None):
    """Box-head training feeder: points [P,D] f64 pool, seg_offsets [S+1] int32 CSR, centers [S,D] f64,
    extra [S] f64 or None -> (x [S,input_size,D(+1)] f32, count [S] int32)."""
    points = _dev(points, torch.float64, "points")
    seg_offsets = _dev(seg_offsets, torch.int32, "seg_offsets")
    centers = _dev(centers, torch.float64, "centers")
    if extra is not None:
        extra = _dev(extra, torch.float64, "extra")
    D = points.shape[1]
    S = seg_offsets.numel() - 1
    if centers.shape != (S, D):
        raise ValueError("centers must be [S, D]")
    if max_segment is None:
        max_segment = int((seg_offsets[1:] - seg_offsets[:-1]).max().item()) if S > 0 else 0
    W = D + (0 if extra is None else 1)
    x = torch.zeros((S, int(input_size), W), dtype=torch.float32, device=points.device)
    count = torch.zeros((S,), dtype=torch.int32, device=points.device)
    if S > 0:
        with torch.cuda.device(points.device):
            _lib.call("pof_segment_resample", _ptr(points), D, _ptr(seg_offsets), S, int(max_segment), _ptr(centers),
                      _ptr(extra) if extra is not None else None, float(random_drop), int(input_size),
                      int(seed) & 0xFFFFFFFF, _ptr(x), _ptr(count), _stream())
    return x, count


def polar_grid(scans, min_range=0.0, max_range=30.0, range_bin_size=1.0, tsdf_clip=1.0, normalize=True, out=None):
    """N4 for a batch: scans [B,T,N] float32 -> [B, T, R, N] float32, R = int((max-min)/bin) + 1."""
    scans = _dev(scans, torch.float32, "scans")
    if scans.dim() != 3:
        raise ValueError("scans must be [B,T,N]")
    B, T, N = scans.shape
    R = int((max_range - min_range) / range_bin_size) + 1
    if out is None:
        out = torch.empty((B, T, R, N), dtype=torch.float32, device=scans.device)
    else:
        _dev(out, torch.float32, "out")
        if tuple(out.shape) != (B, T, R, N):
            raise ValueError("out has the wrong shape")
    with torch.cuda.device(scans.device):
        _lib.call("pof_polar_grid", _ptr(scans), B, T, N, float(min_range), float(max_range), float(range_bin_size),
                  float(tsdf_clip), int(bool(normalize)), _ptr(out), _stream())
    return out


def nms_predicted_center(ranges, tab, pred_cls, pred_reg, min_dist=0.5):
    """A11 batched: ranges [B,N] f32, pred_cls [B,N] f64, pred_reg [B,N,2] f64 ->
    (det_xy [B,N,2], det_cls [B,N], num_det [B] int32, instance_mask [B,N] int32)."""
    ranges = _dev(ranges, torch.float32, "ranges")
    B, N = ranges.shape
    pred_cls = _dev(pred_cls, torch.float64, "pred_cls")
    pred_reg = _dev(pred_reg, torch.float64, "pred_reg")
    if tuple(pred_cls.shape) != (B, N) or tuple(pred_reg.shape) != (B, N, 2):
        raise AssertionError("pred_cls must be [B,N] and pred_reg [B,N,2]")
    dev = ranges.device
    det_xy = torch.zeros((B, N, 2), dtype=torch.float64, device=dev)
    det_cls = torch.zeros((B, N), dtype=torch.float64, device=dev)
    num = torch.zeros(B, dtype=torch.int32, device=dev)
    inst = torch.zeros((B, N), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.call("pof_nms_predicted_center", _ptr(ranges), _ptr(tab), _ptr(pred_cls), _ptr(pred_reg),
                  float(min_dist), B, N, _ptr(det_xy), _ptr(det_cls), _ptr(num), _ptr(inst), None, 0,
                  _stream())
    return det_xy, det_cls, num, inst


# ---------------------------------------------------------------------------------------------------------------------
# The per-scan stages N5-N18.  Each keeps its tensors in records: a namedtuple class declared once by ``_record``, with
# a dtype and a symbolic shape per field.  ``_zeros_of`` allocates a record, ``_checked`` takes a caller's and
# ``_out_of`` does whichever an ``out=`` needs; ``stage_settings`` reads a wrapper's tunable scalars off its signature.
def _record(name, persistent=None, **fields):
    """The namedtuple class ``name`` with one field per keyword, in their order: field=(dtype, *dims), a dim being a
    number or the name of a size ("B" sensors, "N" points, "K" keys or rotations, "M" track slots, "H" x "W" cells, "T"
    translations per axis).  The fields of
    the dict ``persistent`` come first and are the ones that carry over from scan to scan (``cls.persistent``, their
    names); ``cls.spec`` is the (dtype, dims) of every field."""
    fields = dict(persistent or {}, **fields)
    cls = collections.namedtuple(name, tuple(fields))
    cls.spec = tuple((dt, dims) for dt, *dims in fields.values())
    cls.persistent = tuple(persistent or ())
    return cls


@functools.lru_cache(maxsize=256)
def _shapes_of(cls, **sizes):
    """The shape of every field of the record ``cls`` for the given sizes (B=..., N=...).  Cached: a stage is called
    with the same sizes scan after scan, and the per-call checks then resolve no name."""
    return tuple(tuple(sizes.get(d, d) for d in dims) for _, dims in cls.spec)


def _zeros_of(cls, device, **sizes):
    """The record ``cls`` of zero-filled tensors for the given sizes."""
    return cls(*(torch.zeros(shape, dtype=dt, device=device)
                 for (dt, _), shape in zip(cls.spec, _shapes_of(cls, **sizes))))


def _checked(cls, tensors, prefix, **sizes):
    """A caller's tensors as the record ``cls``: each on the device, of its dtype, contiguous and of its shape for the
    given sizes; an error names ``prefix.field``."""
    rec = tensors if type(tensors) is cls else cls(*tensors)
    for name, (dt, _), shape, t in zip(cls._fields, cls.spec, _shapes_of(cls, **sizes), rec):
        _dev(t, dt, prefix + "." + name)
        if t.shape != shape:
            raise ValueError("%s.%s has the wrong shape" % (prefix, name))
    return rec


def _out_of(cls, out, device, **sizes):
    """A stage's ``out=``: the caller's record, checked, or a fresh one."""
    return _zeros_of(cls, device, **sizes) if out is None else _checked(cls, out, "out", **sizes)


_STAGE_TENSORS = frozenset(("init", "xy", "weight", "instance_mask", "num_det", "det_xy", "det_cls", "out", "rot", "trans",
                            "flow_trans", "table"))
REQUIRED = inspect.Parameter.empty


def stage_settings(wrapper):
    """The settings of a per-scan stage -- the keyword-only arguments of its wrapper (``scan_match``, ``track_update``,
    ...) that are scalars a user tunes, not tensors -- with the defaults its signature gives them: a fresh {name:
    default}, ``REQUIRED`` for a setting without one.  What wraps a stage (``StreamingDetector``, the classes of
    ``utils``) takes its known names and defaults from here."""
    return {k: p.default for k, p in inspect.signature(wrapper).parameters.items()
            if p.kind is p.KEYWORD_ONLY and k not in _STAGE_TENSORS}


def _scan_input(ranges, tab, name="ranges", least=0):
    """ranges [B,N] float32 (N >= ``least``) matching the angle table -> (ranges, tab, B, N, device)."""
    ranges = _dev(ranges, torch.float32, name)
    if ranges.dim() != 2:
        raise ValueError("%s must be [B,N]" % name)
    B, N = ranges.shape
    if N < least or _dev(tab, torch.float64, "tab").numel() != 3 * N:
        raise ValueError("%s must be [B,N] matching the angle table" % name)
    return ranges, tab, B, N, ranges.device


def _nms_results(instance_mask, num_det, det_xy, det_cls, B, N):
    """The four results of ``nms_predicted_center`` a per-person stage needs, checked for B scans of N points."""
    instance_mask = _dev(instance_mask, torch.int32, "instance_mask")
    num_det = _dev(num_det, torch.int32, "num_det")
    det_xy = _dev(det_xy, torch.float64, "det_xy")
    det_cls = _dev(det_cls, torch.float64, "det_cls")
    if tuple(instance_mask.shape) != (B, N) or tuple(num_det.shape) != (B,) or tuple(det_xy.shape) != (B, N, 2) or \
            tuple(det_cls.shape) != (B, N):
        raise ValueError("instance_mask and det_cls must be [B,N], num_det [B] and det_xy [B,N,2]")
    return instance_mask, num_det, det_xy, det_cls


_F32, _F64, _I32, _I16, _U8 = torch.float32, torch.float64, torch.int32, torch.int16, torch.uint8
PersonFlow = _record("PersonFlow", flow_global=(_F32, "B", "N", 2), flow_world=(_F64, "B", "N", 2),
                     rgb=(_F64, "B", "N", 3), det_xy_world=(_F64, "B", "N", 2), det_flow=(_F64, "B", "N", 2),
                     det_rgb=(_F64, "B", "N", 3), det_count=(_I32, "B", "N"), det_valid=(_U8, "B", "N"))


def person_flow_buffers(B, N, device="cuda"):
    """The eight outputs of ``person_flow`` for B scans of N points, zero-filled, as its ``out=`` (allocate once,
    before a graph capture)."""
    return _zeros_of(PersonFlow, device, B=B, N=N)


def person_flow(flow_canonical, tab, instance_mask, num_det, det_xy, det_cls, rot=None, trans=None, flow_trans=None,
                cls_thresh=0.5, out=None):
    """N5: per-person flow in the world frame, one launch per batch (depracted_scripts/infer_person_flow.py:134-157).

    flow_canonical [B,N,2] f32 (a flow net's output); instance_mask [B,N] i32, num_det [B] i32, det_xy [B,N,2] f64,
    det_cls [B,N] f64 as ``nms_predicted_center`` returns them.  Sensor pose per scan: rot [B,2,2] (or [B,4]) f32 =
    ``_phi_to_rotation_matrix(odom1[2])``, trans [B,2] f64 = ``odom1[:2]``, flow_trans [B,2] f64 =
    ``(odom1 - odom0)[:2]``; the defaults (identity / zeros) leave everything in the scanner frame.
    -> ``PersonFlow``: flow_global [B,N,2] f32, flow_world [B,N,2] f64, rgb [B,N,3] f64 per point; det_xy_world
    [B,N,2], det_flow [B,N,2], det_rgb [B,N,3] f64, det_count [B,N] i32, det_valid [B,N] u8 per detection (rows
    >= num_det[b] are zeros; a detection without points has count 0 and NaN means).  The per-detection means are
    sequential float64 sums in point order: the same bits in every run.  ``out``: a ``PersonFlow`` of preallocated
    tensors (``person_flow_buffers``)."""
    flow_canonical = _dev(flow_canonical, torch.float32, "flow_canonical")
    if flow_canonical.dim() != 3 or flow_canonical.shape[-1] != 2:
        raise ValueError("flow_canonical must be [B,N,2]")
    B, N = flow_canonical.shape[:2]
    dev = flow_canonical.device
    if _dev(tab, torch.float64, "tab").numel() != 3 * N:
        raise ValueError("flow_canonical must be [B,N,2] matching the angle table")
    instance_mask, num_det, det_xy, det_cls = _nms_results(instance_mask, num_det, det_xy, det_cls, B, N)
    _check_pose_terms(B, rot, trans, flow_trans)
    if rot is None:
        rot = torch.eye(2, dtype=torch.float32, device=dev).repeat(B, 1, 1)
    trans, flow_trans = (torch.zeros((B, 2), dtype=torch.float64, device=dev) if t is None else t
                         for t in (trans, flow_trans))
    out = _out_of(PersonFlow, out, dev, B=B, N=N)
    # no early return at B == 0, unlike the stages below: an empty batch goes to the launcher, as it always has
    with torch.cuda.device(dev):
        _lib.call("pof_person_flow", _ptr(flow_canonical), _ptr(tab), _ptr(instance_mask), _ptr(num_det), _ptr(det_xy),
                  _ptr(det_cls), _ptr(rot), _ptr(trans), _ptr(flow_trans), float(cls_thresh), B, N,
                  *[_ptr(t) for t in out], _stream())
    return out


def _nms_gate(instance_mask, num_det, det_cls, B=None, N=None, strict=False):
    """The NMS results that gate people out of a fit.  Without B and N (before any tensor is looked at): only that
    instance_mask comes with the other two.  With them -> the three tensors, checked, or three Nones.  ``strict``
    refuses a num_det or det_cls that would pass unused, without an instance_mask: for the stages that also report per
    detection (the map stages)."""
    if instance_mask is None:
        if strict and (num_det is not None or det_cls is not None):
            raise ValueError("instance_mask, num_det and det_cls (the NMS results) come together or not at all")
        return None, None, None
    if num_det is None or det_cls is None:
        raise ValueError("instance_mask needs num_det and det_cls (the NMS results)")
    if B is None:
        return instance_mask, num_det, det_cls
    instance_mask = _dev(instance_mask, torch.int32, "instance_mask")
    num_det = _dev(num_det, torch.int32, "num_det")
    det_cls = _dev(det_cls, torch.float64, "det_cls")
    if tuple(instance_mask.shape) != (B, N) or tuple(num_det.shape) != (B,) or tuple(det_cls.shape) != (B, N):
        raise ValueError("instance_mask and det_cls must be [B,N] and num_det [B]")
    return instance_mask, num_det, det_cls


def _check_pose_terms(B, rot, trans, flow_trans):
    """The optional pose terms ``person_flow`` reads, as ``pose_advance`` and the keyframe matchers write them."""
    if rot is not None and tuple(_dev(rot, torch.float32, "rot").shape) not in ((B, 2, 2), (B, 4)):
        raise ValueError("rot must be [B,2,2] (or [B,4] row-major)")
    for t, name in ((trans, "trans"), (flow_trans, "flow_trans")):
        if t is not None and tuple(_dev(t, torch.float64, name).shape) != (B, 2):
            raise ValueError("%s must be [B,2]" % name)


def _pose_input(B, rot, trans, *pose):
    """The pose terms a stage cannot do without, checked: rot and trans, and pose [B,3] where the stage takes one."""
    if rot is None or trans is None or any(p is None for p in pose):
        raise TypeError("%s must be tensors on the HIP device (no CPU path)"
                        % ("rot, trans and pose" if pose else "rot and trans"))
    _check_pose_terms(B, rot, trans, None)
    if pose and tuple(_dev(pose[0], torch.float64, "pose").shape) != (B, 3):
        raise ValueError("pose must be [B,3]")


def _grid_state(state, B):
    """A caller's ``GridMapState`` for B sensors, checked -> (state, H, W)."""
    state = GridMapState(*state)
    if not isinstance(state.grid, torch.Tensor) or state.grid.dim() != 3:
        raise TypeError("state.grid must be a [B,H,W] tensor on the HIP device (no CPU path)")
    H, W = state.grid.shape[1:]
    return _checked(GridMapState, state, "state", B=B, H=H, W=W), H, W


def grid_shape(size):
    """The (H, W) of an occupancy grid from a ``size`` setting, one number or a pair: multiples of 64 in [64, 2048],
    the launchers' rule (csrc/pof_grid.h), or this raises.  What wraps a map stage checks its setting here."""
    shape = tuple(int(s) for s in ((size, size) if np.ndim(size) == 0 else size))
    if len(shape) != 2 or any(s % 64 or not 64 <= s <= 2048 for s in shape):
        raise ValueError("size must be a multiple of 64 in [64, 2048] (or two of them, (H, W))")
    return shape


def _check_matcher_settings(window, iters, **not_negative):
    """The settings ``scan_match`` and ``keyframe_match`` share; the keywords, in their order, must be >= 0."""
    if not 1 <= int(window) <= 64:
        raise ValueError("window must be in [1, 64]")
    if not 1 <= int(iters) <= 32:
        raise ValueError("iters must be in [1, 32]")
    for name, v in not_negative.items():
        if not float(v) >= 0.0:
            raise ValueError("%s must be >= 0" % name)


# what every motion fit reports per scan; the two scan matchers' part; what they report per point
_FIT = dict(motion=(_F64, "B", 3), count=(_I32, "B"), rms=(_F64, "B"), ok=(_U8, "B"))
_ICP = dict(_FIT, iters_used=(_I32, "B"), obs=(_F64, "B"))
_ICP_POINTS = dict(corr=(_I32, "B", "N"), flow_residual=(_F64, "B", "N", 2))
EgoMotion = _record("EgoMotion", **_FIT, flow_residual=(_F64, "B", "N", 2), weight=(_F32, "B", "N"))
_EGO_MODELS = {"rigid": 0, "linear": 1}


def ego_motion_buffers(B, N, device="cuda"):
    """The six outputs of ``ego_motion`` for B scans of N points, zero-filled, as its ``out=`` (allocate once, before
    a graph capture)."""
    return _zeros_of(EgoMotion, device, B=B, N=N)


def ego_motion(ranges, tab, flow, *, xy=None, canonical=True, sign=-1, model="rigid", weight=None, instance_mask=None,
               num_det=None, det_cls=None, cls_thresh=0.5, max_range=20.0, huber_delta=0.0, iters=0, out=None):
    """N6: the sensor's own motion from a flow field, one launch per batch -- the weighted least-squares inverse of
    ``get_displacement_from_odometry`` / ``get_velocity_from_odometry`` (src/utils/utils.py:639-662, :609-636).

    ranges [B,N] f32 (or None with ``xy`` [B,N,2] f64: exact points; with both, the ranges only gate), tab the angle
    table (may be None with xy and ``canonical=False``), flow [B,N,2] f32 or f64, canonical or scanner frame.
    ``sign``: q = p + sign * flow is where the point was (-1, the reference's displacement) or will be (+1).
    ``model``: "rigid" -> motion = (theta, u_x, u_y) with q = R(theta) p + u, exact for any angle; "linear" -> motion =
    (omega, t_x, t_y) with sign * flow = t + omega * (-y, x).  weight [B,N] f32 (<= 0 or not finite: excluded).  Points
    with a range >= ``max_range`` or not finite, a flow that is not finite, or -- given the NMS results instance_mask
    [B,N] i32, num_det [B] i32, det_cls [B,N] f64 -- a detection of score >= ``cls_thresh`` are excluded.
    ``huber_delta`` > 0 re-weights ``iters`` (0..16) times by min(1, delta / residual).
    -> ``EgoMotion``: motion [B,3] f64 (NaN when the fit failed: fewer than two points, or all at one place), count
    [B] i32 points used, rms [B] f64, ok [B] u8, flow_residual [B,N,2] f64 (the flow with the sensor's motion taken
    out, scanner frame), weight [B,N] f32 (the last solve's).  Fixed summation order: the same bits in every run.
    ``out``: an ``EgoMotion`` of preallocated tensors (``ego_motion_buffers``)."""
    if ranges is None and xy is None:
        raise ValueError("ego_motion needs ranges or xy")
    if sign not in (-1, 1):
        raise ValueError("sign must be -1 or +1")
    if model not in _EGO_MODELS:
        raise ValueError("model must be 'rigid' or 'linear'")
    if not 0 <= int(iters) <= 16:
        raise ValueError("iters must be in [0, 16]")
    _nms_gate(instance_mask, num_det, det_cls)
    # the one stage whose batch is sized by the flow, float32 or float64: the ranges are optional beside ``xy``
    if not isinstance(flow, torch.Tensor) or flow.dtype not in (torch.float32, torch.float64):
        raise TypeError("flow must be a float32 or float64 tensor on the HIP device (no CPU path)")
    flow = _dev(flow, flow.dtype, "flow")
    if flow.dim() != 3 or flow.shape[-1] != 2:
        raise ValueError("flow must be [B,N,2]")
    B, N = flow.shape[:2]
    dev = flow.device
    if ranges is not None and tuple(_dev(ranges, torch.float32, "ranges").shape) != (B, N):
        raise ValueError("ranges must be [B,N]")
    if xy is not None and tuple(_dev(xy, torch.float64, "xy").shape) != (B, N, 2):
        raise ValueError("xy must be [B,N,2]")
    if tab is None:
        if canonical or xy is None:
            raise ValueError("the angle table is needed for a canonical flow and to place ranges")
    elif _dev(tab, torch.float64, "tab").numel() != 3 * N:
        raise ValueError("flow must be [B,N,2] matching the angle table")
    if weight is not None and tuple(_dev(weight, torch.float32, "weight").shape) != (B, N):
        raise ValueError("weight must be [B,N]")
    instance_mask, num_det, det_cls = _nms_gate(instance_mask, num_det, det_cls, B, N)
    out = _out_of(EgoMotion, out, dev, B=B, N=N)
    if B == 0:
        return out
    with torch.cuda.device(dev):
        _lib.call("pof_ego_motion", _ptr(ranges), _ptr(xy), _ptr(tab), _ptr(flow), int(flow.dtype == torch.float64),
                  int(bool(canonical)), int(sign), _EGO_MODELS[model], _ptr(weight), _ptr(instance_mask), _ptr(num_det),
                  _ptr(det_cls), float(cls_thresh), float(max_range), float(huber_delta), int(iters), B, N,
                  *[_ptr(t) for t in out], _stream())
    return out


def pose_advance(motion, ok, pose, rot=None, trans=None, flow_trans=None):
    """Compose the rigid motion ``ego_motion`` fitted (``sign=-1``, displacement convention) onto pose [B,3] f64 =
    (x, y, phi), IN PLACE: phi += theta, (x, y) += R(phi) u; a scan with ok = 0 keeps its pose.  Optionally writes the
    pose terms ``person_flow`` reads: rot [B,2,2] (or [B,4]) f32, trans [B,2] f64 and flow_trans [B,2] f64 (the
    translation of this step; zeros without ok).  -> pose."""
    motion = _dev(motion, torch.float64, "motion")
    ok = _dev(ok, torch.uint8, "ok")
    pose = _dev(pose, torch.float64, "pose")
    B = pose.shape[0] if pose.dim() == 2 else -1
    if tuple(pose.shape) != (B, 3) or tuple(motion.shape) != (B, 3) or tuple(ok.shape) != (B,):
        raise ValueError("motion and pose must be [B,3] and ok [B]")
    _check_pose_terms(B, rot, trans, flow_trans)
    if B == 0:
        return pose
    with torch.cuda.device(pose.device):
        _lib.call("pof_pose_advance", _ptr(motion), _ptr(ok), _ptr(pose), _ptr(rot), _ptr(trans), _ptr(flow_trans), B,
                  _stream())
    return pose


ScanMatch = _record("ScanMatch", **_ICP, **_ICP_POINTS)


def scan_match_buffers(B, N, device="cuda"):
    """The eight outputs of ``scan_match`` for B scan pairs of N points, zero-filled, as its ``out=`` (allocate once,
    before a graph capture)."""
    return _zeros_of(ScanMatch, device, B=B, N=N)


def scan_match(ranges_prev, ranges_cur, tab, *, init=None, instance_mask=None, num_det=None, det_cls=None,
               cls_thresh=0.5, max_range=20.0, window=16, gate=0.5, max_gap=0.3, huber_delta=0.05, iters=16,
               eps_theta=1e-7, eps_u=1e-7, min_pivot=1e-6, out=None):
    """N8: the sensor's own motion between two consecutive scans without a flow field -- a point-to-line ICP of the
    current scan against the previous one, one launch per batch (include/pof_abi.h states the algorithm).

    ranges_prev, ranges_cur [B,N] f32, tab the angle table.  ``init`` [B,3] f64 = (theta, u_x, u_y) to start from
    (None, or a row that is not finite: zeros; it may be ``out.motion`` of the previous step).  Given the NMS results
    of the current scan -- instance_mask [B,N] i32, num_det [B] i32, det_cls [B,N] f64 -- the points of detections with
    a score >= ``cls_thresh`` do not vote.  Ranges >= ``max_range`` or not finite are left out.  ``window`` (1..64): a
    point looks for its vertex that many beams either side of where the rotation puts it; ``gate`` / ``max_gap``
    (metres): the largest point-to-vertex distance and the longest line segment; ``huber_delta`` (metres, 0: plain);
    ``iters`` (1..32) with the early exit ``eps_theta`` / ``eps_u``; ``min_pivot``: the smallest Cholesky pivot, as a
    fraction of the largest diagonal entry, below which the pair fails (a corridor).
    -> ``ScanMatch``: motion [B,3] f64 with q = R(theta) p + u where the point now at p was (the convention of
    ``ego_motion``'s rigid model: ``pose_advance`` takes it), NaN when the pair failed; count [B] i32 matched points,
    rms [B] f64, ok [B] u8, iters_used [B] i32, obs [B] f64 (smallest pivot / largest diagonal entry), corr [B,N] i32
    (the matched vertex or -1) and flow_residual [B,N,2] f64 (the motion-compensated nearest-vertex displacement in
    the current scanner frame, NaN where unmatched).  Fixed summation order: the same bits in every run.
    ``out``: a ``ScanMatch`` of preallocated tensors (``scan_match_buffers``)."""
    _check_matcher_settings(window, iters, gate=gate, max_gap=max_gap, huber_delta=huber_delta)
    _nms_gate(instance_mask, num_det, det_cls)
    ranges_cur = _dev(ranges_cur, torch.float32, "ranges_cur")
    ranges_prev = _dev(ranges_prev, torch.float32, "ranges_prev")
    if ranges_prev.shape != ranges_cur.shape:
        raise ValueError("ranges_prev and ranges_cur must be [B,N]")
    ranges_cur, tab, B, N, dev = _scan_input(ranges_cur, tab, "ranges_cur", least=1)    # a matcher refuses N < 1
    if init is not None and tuple(_dev(init, torch.float64, "init").shape) != (B, 3):
        raise ValueError("init must be [B,3]")
    instance_mask, num_det, det_cls = _nms_gate(instance_mask, num_det, det_cls, B, N)
    out = _out_of(ScanMatch, out, dev, B=B, N=N)
    if B == 0:
        return out
    with torch.cuda.device(dev):
        _lib.call("pof_scan_match", _ptr(ranges_prev), _ptr(ranges_cur), _ptr(tab), _ptr(init), _ptr(instance_mask),
                  _ptr(num_det), _ptr(det_cls), float(cls_thresh), float(max_range), int(window), float(gate),
                  float(max_gap), float(huber_delta), int(iters), float(eps_theta), float(eps_u), float(min_pivot),
                  B, N, *[_ptr(t) for t in out], _stream())
    return out


KeyframeState = _record("KeyframeState", key_ranges=(_F32, "B", "N"), key_pose=(_F64, "B", 3), key_rel=(_F64, "B", 3),
                        key_valid=(_U8, "B"), key_age=(_I32, "B"), key_misses=(_I32, "B"), pose=(_F64, "B", 3))
KeyframeMatch = _record("KeyframeMatch", **_ICP, key_replaced=(_U8, "B"), **_ICP_POINTS)


def _keyframe_reset(state, pose):
    """Zero every tensor of a keyframe state but ``pose`` (its last field), which takes ``pose`` or zeros."""
    for t in state[:-1]:
        t.zero_()
    if pose is None:
        state.pose.zero_()
    else:
        pose = torch.as_tensor(pose, dtype=torch.float64).reshape(-1, 3)
        state.pose.copy_(pose.expand(state.pose.shape[0], 3), non_blocking=True)
    return state


def _keyframe_step(entry, State, Out, ranges_cur, tab, state, instance_mask, num_det, det_cls, cls_thresh,
                   max_range, window, gate, max_gap, huber_delta, iters, eps_theta, eps_u, min_pivot, key_dist, key_rot,
                   min_share, max_misses, out, rot, trans, flow_trans, revisit=None):
    """``keyframe_match`` (``revisit`` None) and ``keyframe_map_match``: the checks and the call of ``entry``, for the
    records ``State`` and ``Out``.  With a ring the state's shapes also take K, read off state.key_ranges [B,K,N], and
    the entry point takes ``revisit`` in front of B and K behind N."""
    _check_matcher_settings(window, iters, gate=gate, max_gap=max_gap, huber_delta=huber_delta, key_dist=key_dist,
                            key_rot=key_rot, min_share=min_share)
    if int(max_misses) < 0:
        raise ValueError("max_misses must be >= 0")
    if revisit is not None and not 0.0 <= float(revisit) <= 1.0:
        raise ValueError("revisit must be in [0, 1]")
    _nms_gate(instance_mask, num_det, det_cls)
    ranges_cur, tab, B, N, dev = _scan_input(ranges_cur, tab, "ranges_cur", least=1)    # a matcher refuses N < 1
    state = State(*state)
    ring = {}
    if revisit is not None:
        if not isinstance(state.key_ranges, torch.Tensor) or state.key_ranges.dim() != 3:
            raise ValueError("state.key_ranges must be [B,K,N]")
        ring = dict(K=_check_keys(state.key_ranges.shape[1]))
    state = _checked(State, state, "state", B=B, N=N, **ring)
    instance_mask, num_det, det_cls = _nms_gate(instance_mask, num_det, det_cls, B, N)
    out = _out_of(Out, out, dev, B=B, N=N)
    _check_pose_terms(B, rot, trans, flow_trans)
    if B == 0:
        return out
    with torch.cuda.device(dev):
        _lib.call(entry, _ptr(ranges_cur), _ptr(tab), _ptr(instance_mask), _ptr(num_det), _ptr(det_cls),
                  float(cls_thresh), float(max_range), int(window), float(gate), float(max_gap), float(huber_delta),
                  int(iters), float(eps_theta), float(eps_u), float(min_pivot), float(key_dist), float(key_rot),
                  float(min_share), int(max_misses), *(() if revisit is None else (float(revisit),)), B, N, *ring.values(),
                  *[_ptr(t) for t in state], *[_ptr(t) for t in out], _ptr(rot), _ptr(trans), _ptr(flow_trans),
                  _stream())
    return out


def keyframe_buffers(B, N, device="cuda"):
    """The persistent state of ``keyframe_match`` for B sensors of N points: no keyframe yet, the pose at zero
    (allocate once, before a graph capture).  -> ``KeyframeState``."""
    return _zeros_of(KeyframeState, device, B=B, N=N)


def keyframe_match_buffers(B, N, device="cuda"):
    """The nine outputs of ``keyframe_match``, zero-filled, as its ``out=``."""
    return _zeros_of(KeyframeMatch, device, B=B, N=N)


def keyframe_reset(state, pose=None):
    """Forget the keyframe of every sensor, IN PLACE and without a synchronisation: the next ``keyframe_match`` seeds.
    pose ([3] or [B,3]): the pose to go on from; zeros by default."""
    return _keyframe_reset(KeyframeState(*state), pose)


def keyframe_match(ranges_cur, tab, state, *, instance_mask=None, num_det=None, det_cls=None, cls_thresh=0.5,
                   max_range=20.0, window=16, gate=0.5, max_gap=0.3, huber_delta=0.05, iters=16, eps_theta=1e-7,
                   eps_u=1e-7, min_pivot=1e-6, key_dist=0.3, key_rot=0.3, min_share=0.5, max_misses=2, out=None,
                   rot=None, trans=None, flow_trans=None):
    """N9: one step of keyframe scan matching -- the current scan is matched against the sensor's keyframe (a
    point-to-line ICP as ``scan_match``, the window of a point centred on the beam it projects to), the pose becomes
    key_pose o (theta, u), and the keyframe is replaced on the device when the sensor has left it; one launch per
    batch (include/pof_abi.h states the algorithm).

    ranges_cur [B,N] f32, tab the angle table, ``state`` a ``KeyframeState`` (``keyframe_buffers``), UPDATED IN PLACE:
    a sensor without a keyframe (``key_valid`` 0) takes this scan as its keyframe and reports ok = 0.  The NMS results
    gate people as in ``scan_match``, also out of a scan that becomes the keyframe.  The settings up to ``min_pivot``
    are ``scan_match``'s.  The keyframe is replaced by the current scan when the match has |theta| > ``key_rot``
    (radians), |u| > ``key_dist`` (metres) or fewer matched points than ``min_share`` of the points that vote, and
    after more than ``max_misses`` failed matches in a row (at the unchanged pose).
    -> ``KeyframeMatch``: motion [B,3] f64 = (theta, u) against the keyframe that was matched (NaN without ok), count,
    rms, ok, iters_used, obs as ``scan_match``, key_replaced [B] u8, corr [B,N] i32 and flow_residual [B,N,2] f64.
    ``out``: a ``KeyframeMatch`` of preallocated tensors (``keyframe_match_buffers``).  ``rot`` [B,2,2] (or [B,4]) f32,
    ``trans`` [B,2] f64, ``flow_trans`` [B,2] f64: the pose terms ``person_flow`` reads, as ``pose_advance`` writes
    them."""
    return _keyframe_step("pof_keyframe_match", KeyframeState, KeyframeMatch, ranges_cur, tab, state, instance_mask,
                          num_det, det_cls, cls_thresh, max_range, window, gate, max_gap, huber_delta, iters, eps_theta,
                          eps_u, min_pivot, key_dist, key_rot, min_share, max_misses, out, rot, trans, flow_trans)


KeyframeMapState = _record("KeyframeMapState", key_ranges=(_F32, "B", "K", "N"), key_pose=(_F64, "B", "K", 3),
                           key_valid=(_U8, "B", "K"), key_stamp=(_I32, "B", "K"), key_active=(_I32, "B"),
                           key_rel=(_F64, "B", 3), key_age=(_I32, "B"), key_misses=(_I32, "B"), step=(_I32, "B"),
                           pose=(_F64, "B", 3))
KeyframeMapMatch = _record("KeyframeMapMatch", **_ICP, key_replaced=(_U8, "B"), key_switched=(_U8, "B"),
                           key_slot=(_I32, "B"), **_ICP_POINTS)


def _check_keys(keys):
    if not 1 <= int(keys) <= 64:
        raise ValueError("keys must be in [1, 64]")
    return int(keys)


def keyframe_map_buffers(B, N, keys=16, device="cuda"):
    """The persistent state of ``keyframe_map_match`` for B sensors of N points and a ring of ``keys`` (1..64)
    keyframes each: no keyframe yet, slot 0 active, the pose at zero (allocate once, before a graph capture).
    -> ``KeyframeMapState``."""
    return _zeros_of(KeyframeMapState, device, B=B, N=N, K=_check_keys(keys))


def keyframe_map_match_buffers(B, N, device="cuda"):
    """The eleven outputs of ``keyframe_map_match``, zero-filled, as its ``out=``."""
    return _zeros_of(KeyframeMapMatch, device, B=B, N=N)


def keyframe_map_reset(state, pose=None):
    """Forget every keyframe of every sensor, IN PLACE and without a synchronisation: slot 0 is active, the scan
    counter restarts and the next ``keyframe_map_match`` seeds.  pose ([3] or [B,3]): the pose to go on from; zeros by
    default."""
    return _keyframe_reset(KeyframeMapState(*state), pose)


def keyframe_map_match(ranges_cur, tab, state, *, instance_mask=None, num_det=None, det_cls=None, cls_thresh=0.5,
                       max_range=20.0, window=16, gate=0.5, max_gap=0.3, huber_delta=0.05, iters=16, eps_theta=1e-7,
                       eps_u=1e-7, min_pivot=1e-6, key_dist=0.3, key_rot=0.3, min_share=0.5, max_misses=2, revisit=0.5,
                       out=None, rot=None, trans=None, flow_trans=None):
    """N10: one step of keyframe matching against a ring of keyframes per sensor -- ``keyframe_match`` on the active
    keyframe, and when the sensor leaves it, it switches to a stored keyframe it has come back to instead of storing a
    new one, so the next match re-anchors the pose there and the drift of the way round is dropped; one launch per
    batch (include/pof_abi.h states the algorithm).

    ranges_cur [B,N] f32, tab the angle table, ``state`` a ``KeyframeMapState`` (``keyframe_map_buffers``; its
    key_ranges [B,K,N] gives the ring size K), UPDATED IN PLACE.  The settings up to ``max_misses`` are
    ``keyframe_match``'s.  A stored keyframe counts as revisited when the pose just formed lies within ``revisit``
    (0..1) times ``key_rot`` and ``key_dist`` of it; the nearest such keyframe becomes the active one.  Without one the
    scan is stored in a free slot, else over the slot that has not been active for the longest time.
    -> ``KeyframeMapMatch``: the outputs of ``keyframe_match`` and key_switched [B] u8, key_slot [B] i32 (the active
    slot after the step).  ``out``: a ``KeyframeMapMatch`` of preallocated tensors (``keyframe_map_match_buffers``);
    ``rot``, ``trans``, ``flow_trans`` as ``keyframe_match``."""
    return _keyframe_step("pof_keyframe_map_match", KeyframeMapState, KeyframeMapMatch, ranges_cur, tab, state,
                          instance_mask, num_det, det_cls, cls_thresh, max_range, window, gate, max_gap, huber_delta,
                          iters, eps_theta, eps_u, min_pivot, key_dist, key_rot, min_share, max_misses, out, rot, trans,
                          flow_trans, revisit=revisit)


# the tracks themselves carry over from scan to scan; the rest describes one step (M: slot, N: detection row / point)
TrackState = _record("TrackState",
                     persistent=dict(track_id=(_I32, "B", "M"), track_state=(_F64, "B", "M", 4),
                                     track_cov=(_F64, "B", "M", 3), track_hits=(_I32, "B", "M"),
                                     track_misses=(_I32, "B", "M"), track_age=(_I32, "B", "M"), next_id=(_I32, "B")),
                     track_det=(_I32, "B", "M"), track_confirmed=(_U8, "B", "M"), det_track=(_I32, "B", "N"),
                     point_track=(_I32, "B", "N"), dropped=(_I32, "B"))


def track_buffers(B, max_tracks, N, device="cuda"):
    """The state and the outputs of ``track_update`` for B sensors, ``max_tracks`` slots and N detection rows: a
    ``TrackState`` of zeros with ``next_id`` = 1 (allocate once, before a graph capture)."""
    state = _zeros_of(TrackState, device, B=B, M=int(max_tracks), N=N)
    state.next_id.fill_(1)
    return state


def track_reset(state):
    """Free every track and restart the ids at 1, in place, with tensor ops on the current stream (no host sync)."""
    state = TrackState(*state)
    for t in state:
        t.zero_()
    state.next_id.fill_(1)
    return state


def track_update(det_xy_world, det_flow, det_valid, num_det, instance_mask, state, *, gate=0.5, q=1e-4, r_pos=2.5e-3,
                 r_vel=2.5e-3, v0_var=0.25, max_misses=3, min_hits=3):
    """N7: one step of the person tracks, one launch per batch (include/pof_abi.h has the step in full).

    det_xy_world [B,N,2], det_flow [B,N,2] f64 and det_valid [B,N] u8 as ``person_flow`` returns them, num_det [B] i32
    and instance_mask [B,N] i32 as the NMS does.  ``state``: a ``TrackState`` (``track_buffers``), updated IN PLACE:
    every live track is predicted one scan ahead (centre + velocity), detections inside ``gate`` metres are associated
    greedily by distance (ties: lower slot, lower row), a matched track takes a position update (noise ``r_pos`` m^2) and,
    when the detection's flow is finite, a velocity update (``r_vel``); ``q`` is the velocity process noise per scan.
    An unmatched track is dropped after more than ``max_misses`` misses, an unmatched detection starts a track with
    the flow as its velocity (variance ``v0_var`` without one), and a track counts as confirmed from ``min_hits`` hits.
    -> state; its track_det / track_confirmed / det_track / point_track / dropped describe this step.
    max_tracks <= 256, N <= 4096.  The same bits in every run."""
    det_xy_world = _dev(det_xy_world, torch.float64, "det_xy_world")
    if det_xy_world.dim() != 3 or det_xy_world.shape[-1] != 2:
        raise ValueError("det_xy_world must be [B,N,2]")
    B, N = det_xy_world.shape[:2]
    det_flow = _dev(det_flow, torch.float64, "det_flow")
    det_valid = _dev(det_valid, torch.uint8, "det_valid")
    num_det = _dev(num_det, torch.int32, "num_det")
    instance_mask = _dev(instance_mask, torch.int32, "instance_mask")
    if tuple(det_flow.shape) != (B, N, 2) or tuple(det_valid.shape) != (B, N) or tuple(num_det.shape) != (B,) or \
            tuple(instance_mask.shape) != (B, N):
        raise ValueError("det_flow must be [B,N,2], det_valid and instance_mask [B,N] and num_det [B]")
    state = TrackState(*state)
    if state.track_id.dim() != 2:
        raise ValueError("state.track_id must be [B,max_tracks]")
    M = state.track_id.shape[1]
    state = _checked(TrackState, state, "state", B=B, M=M, N=N)
    if B == 0:
        return state
    with torch.cuda.device(det_xy_world.device):
        _lib.call("pof_track_update", _ptr(det_xy_world), _ptr(det_flow), _ptr(det_valid), _ptr(num_det),
                  _ptr(instance_mask), B, N, M, *[_ptr(t) for t in state], float(gate), float(q), float(r_pos),
                  float(r_vel), float(v0_var), int(max_misses), int(min_hits), _stream())
    return state


PersonMotion = _record("PersonMotion", det_xy_world=(_F64, "B", "N", 2), det_flow=(_F64, "B", "N", 2),
                       det_centre=(_F64, "B", "N", 2), det_count=(_I32, "B", "N"), det_valid=(_U8, "B", "N"),
                       det_prev=(_I32, "B", "N"))
PersonMotionState = _record("PersonMotionState", prev_centre=(_F64, "B", "N", 2), prev_cand=(_U8, "B", "N"),
                            prev_num=(_I32, "B"))


def person_motion_buffers(B, N, device="cuda"):
    """The six outputs of ``person_motion`` for B scans of N points, zero-filled, as its ``out=`` (allocate once,
    before a graph capture)."""
    return _zeros_of(PersonMotion, device, B=B, N=N)


def person_motion_state(B, N, device="cuda"):
    """The persistent state of ``person_motion`` for B sensors of N points: no previous scan (allocate once, before a
    graph capture).  -> ``PersonMotionState``."""
    return _zeros_of(PersonMotionState, device, B=B, N=N)


def person_motion_reset(state):
    """Forget the previous scan of every sensor, in place, with tensor ops on the current stream (no host sync): the
    next ``person_motion`` seeds."""
    state = PersonMotionState(*state)
    for t in state:
        t.zero_()
    return state


def person_motion(ranges, tab, instance_mask, num_det, det_xy, det_cls, rot, trans, state, *, cls_thresh=0.5,
                  max_range=20.0, reach=0.5, min_points=3, out=None):
    """N11: person motion without a flow net, one launch per batch (include/pof_abi.h states the rules in full).

    ranges [B,N] f32, the current scan; tab the angle table; instance_mask [B,N] i32, num_det [B] i32, det_xy [B,N,2]
    f64, det_cls [B,N] f64 as ``nms_predicted_center`` returns them; rot [B,2,2] (or [B,4]) f32 and trans [B,2] f64,
    the sensor's pose at this scan as ``pose_advance`` and the keyframe matchers write it.  ``state``: a
    ``PersonMotionState`` (``person_motion_state``), UPDATED IN PLACE; with ``prev_num`` 0 the launch only seeds.
    Per detection the world-frame centroid of its own scan points (finite ranges < ``max_range``, summed in point
    order) is paired with the previous scan's centroids by a strict mutual-nearest rule within ``reach`` metres; only
    detections of score >= ``cls_thresh`` with at least ``min_points`` points take part.
    -> ``PersonMotion``: det_xy_world [B,N,2] f64 and det_valid [B,N] u8 with the bits of ``person_flow``'s, det_flow
    [B,N,2] f64 = the displacement since the previous scan (NaN without a partner: ``track_update`` then updates the
    position only), det_centre [B,N,2] f64, det_count [B,N] i32, det_prev [B,N] i32 = the partner's row in the previous
    scan or -1.  Rows >= num_det[b] are zeros (det_prev -1).  The same bits in every run.  ``out``: a ``PersonMotion``
    of preallocated tensors (``person_motion_buffers``)."""
    ranges, tab, B, N, dev = _scan_input(ranges, tab)
    instance_mask, num_det, det_xy, det_cls = _nms_results(instance_mask, num_det, det_xy, det_cls, B, N)
    _pose_input(B, rot, trans)
    state = _checked(PersonMotionState, state, "state", B=B, N=N)
    out = _out_of(PersonMotion, out, dev, B=B, N=N)
    if B == 0:
        return out
    with torch.cuda.device(dev):
        _lib.call("pof_person_motion", _ptr(ranges), _ptr(tab), _ptr(instance_mask), _ptr(num_det), _ptr(det_xy),
                  _ptr(det_cls), _ptr(rot), _ptr(trans), float(cls_thresh), float(max_range), float(reach),
                  int(min_points), B, N, *[_ptr(t) for t in state], *[_ptr(t) for t in out], _stream())
    return out


GridMapState = _record("GridMapState", grid=(_I16, "B", "H", "W"), origin=(_F64, "B", 2))
GridMapOut = _record("GridMapOut", point_cell=(_I32, "B", "N"), point_mark=(_U8, "B", "N"), point_prior=(_I16, "B", "N"),
                     det_points=(_I32, "B", "N"), det_free=(_I32, "B", "N"))


def grid_map_buffers(B, N, device="cuda"):
    """The five outputs of ``grid_map_update`` for B scans of N points, zero-filled, as its ``out=`` (allocate once,
    before a graph capture)."""
    return _zeros_of(GridMapOut, device, B=B, N=N)


def grid_map_state(B, H, W, device="cuda"):
    """The persistent state of ``grid_map_update`` for B sensors: a grid of H x W cells, all unknown, with its lower
    corner at the world origin (allocate once, before a graph capture).  -> ``GridMapState``."""
    return _zeros_of(GridMapState, device, B=B, H=H, W=W)


def grid_map_reset(state, origin=None):
    """Every cell unknown again, in place, with tensor ops on the current stream (no host sync).  origin ([2] or [B,2],
    numbers or a device tensor): the world position of the lower corner of cell (0, 0); zeros by default."""
    state = GridMapState(*state)
    state.grid.zero_()
    if origin is None:
        state.origin.zero_()
    else:
        origin = torch.as_tensor(origin, dtype=torch.float64).reshape(-1, 2)
        state.origin.copy_(origin.expand(state.origin.shape[0], 2), non_blocking=True)
    return state


def grid_map_update(ranges, tab, rot, trans, state, *, res, instance_mask=None, num_det=None, det_cls=None,
                    cls_thresh=0.5, max_range=20.0, tol=None, hit=17, miss=8, lo=-40, hi=70, free_thresh=16, out=None):
    """N12: one scan into the occupancy grid of every sensor, two launches per batch (include/pof_abi.h states the
    rules in full).

    ranges [B,N] f32, the current scan; tab the angle table; rot [B,2,2] (or [B,4]) f32 and trans [B,2] f64, the
    sensor's pose at this scan as ``pose_advance`` and the keyframe matchers write it.  ``state``: a ``GridMapState``
    (``grid_map_state``): grid [B,H,W] i16, the log-odds in integer counts (0 = unknown), UPDATED IN PLACE, and origin
    [B,2] f64, the world position of the grid's lower corner; H and W multiples of 64 in [64, 2048].  ``res``: metres
    per cell.  A cell that holds the endpoint of a beam (finite, 0 < r < ``max_range``) gains ``hit``; otherwise a cell
    whose beam and its two neighbours all pass it by more than ``tol`` (None: ``res``) loses ``miss``; the value stays
    in [``lo``, ``hi``].  The defaults read as counts of 0.05 nat.  With the NMS results instance_mask [B,N] i32,
    num_det [B] i32, det_cls [B,N] f64 (all three or none) the points of detections of score >= ``cls_thresh`` are
    never burned in.
    -> ``GridMapOut``: point_cell [B,N] i32 (the cell iy W + ix of every endpoint, -1 without one inside the grid),
    point_mark [B,N] u8 (the endpoint was burned in), point_prior [B,N] i16 (what its cell held before this scan,
    -32768 without one), det_points / det_free [B,N] i32 (per detection row the endpoints inside the grid and how many
    of them lie on cells that held <= -``free_thresh``; zeros without the NMS results).  The same bits in every run.
    ``out``: a ``GridMapOut`` of preallocated tensors (``grid_map_buffers``)."""
    ranges, tab, B, N, dev = _scan_input(ranges, tab)
    _pose_input(B, rot, trans)
    gate = _nms_gate(instance_mask, num_det, det_cls, B, N, strict=True)
    state, H, W = _grid_state(state, B)
    out = _out_of(GridMapOut, out, dev, B=B, N=N)
    if B == 0:
        return out
    with torch.cuda.device(dev):
        _lib.call("pof_grid_map_update", _ptr(ranges), _ptr(tab), _ptr(rot), _ptr(trans), *[_ptr(t) for t in gate],
                  float(res), float(res if tol is None else tol), float(max_range), float(cls_thresh), int(hit),
                  int(miss), int(lo), int(hi), int(free_thresh), B, N, H, W, *[_ptr(t) for t in state],
                  *[_ptr(t) for t in out], _stream())
    return out


GridMatch = _record("GridMatch", scores=(_I32, "B", "K", "T", "T"), best=(_I32, "B", 3), score=(_I32, "B", 2),
                    votes=(_I32, "B"), ok=(_U8, "B"), moved=(_U8, "B"), correction=(_F64, "B", 3))


def _check_search(reach, rotations):
    if not 0 <= int(reach) <= 16:
        raise ValueError("reach must be in [0, 16]")
    if not 1 <= int(rotations) <= 33 or int(rotations) % 2 == 0:
        raise ValueError("rotations must be odd and in [1, 33]")


def grid_match_buffers(B, reach=4, rotations=9, device="cuda"):
    """The seven outputs of ``grid_match`` for B sensors and a search of ``rotations`` x (2 ``reach`` + 1)^2 candidates,
    zero-filled, as its ``out=`` (allocate once, before a graph capture)."""
    _check_search(reach, rotations)
    return _zeros_of(GridMatch, device, B=B, K=int(rotations), T=2 * int(reach) + 1)


def grid_match_table(rot_step=0.01, rotations=9, device="cuda"):
    """The rotation table of ``grid_match`` -> [rotations, 3] f64 = (theta, cos theta, sin theta) with theta_k =
    (k - (rotations - 1) / 2) ``rot_step``, cosines and sines by NumPy; the middle row is exactly (0, 1, 0)."""
    _check_search(0, rotations)
    theta = (np.arange(int(rotations), dtype=np.float64) - (int(rotations) - 1) // 2) * float(rot_step)
    return torch.from_numpy(np.stack([theta, np.cos(theta), np.sin(theta)], axis=1)).to(device)


def grid_match(ranges, tab, rot, trans, pose, state, *, res, table=None, instance_mask=None, num_det=None,
               det_cls=None, cls_thresh=0.5, max_range=20.0, reach=4, rotations=9, rot_step=0.01, min_points=50,
               min_score=20, min_gain=8, out=None):
    """N13: the pose of every sensor corrected against its occupancy grid, two launches per batch (include/pof_abi.h
    states the rules in full).

    ranges [B,N] f32, the current scan; tab the angle table; rot [B,2,2] (or [B,4]) f32, trans [B,2] f64 and pose [B,3]
    f64 = (x, y, phi), the sensor's pose at this scan as ``pose_advance`` leaves it, all three UPDATED IN PLACE when a
    sensor is moved.  ``state``: the ``GridMapState`` of ``grid_map_update``, read only; ``res``: its metres per cell.
    Every point that votes (finite, 0 < r < ``max_range``, no point of a detection of score >= ``cls_thresh`` when the
    NMS results instance_mask [B,N] i32, num_det [B] i32, det_cls [B,N] f64 are given, all three or none) is entered at
    ``rotations`` rotations, ``rot_step`` radians apart around the pose, and (2 ``reach`` + 1)^2 whole-cell
    translations, and the grid values under it are summed, in integers.  The best candidate (ties: the shorter
    translation, the smaller rotation, the lower index) is ``ok`` with at least ``min_points`` voting points and a score
    of at least ``min_score`` per voting point; the sensor is ``moved`` there when it is not the incoming pose and gains
    at least ``min_gain`` per voting point over it.  ``table``: ``grid_match_table(rot_step, rotations)``; None builds
    it, which allocates -- a graph capture passes its own (``rot_step`` is then not read).
    -> ``GridMatch``: scores [B,rotations,T,T] i32, best [B,3] i32 = (rotation, dy, dx) of the best candidate in steps
    and cells, score [B,2] i32 = (the best, the incoming pose's), votes [B] i32, ok [B], moved [B] u8, correction [B,3]
    f64 = (dx res, dy res, theta), zeros without ``moved``.  The same bits in every run.  ``out``: a ``GridMatch`` of
    preallocated tensors (``grid_match_buffers``)."""
    ranges, tab, B, N, dev = _scan_input(ranges, tab)
    _pose_input(B, rot, trans, pose)
    gate = _nms_gate(instance_mask, num_det, det_cls, B, N, strict=True)
    state, H, W = _grid_state(state, B)
    _check_search(reach, rotations)
    if table is None:
        table = grid_match_table(rot_step, rotations, dev)
    if tuple(_dev(table, torch.float64, "table").shape) != (int(rotations), 3):
        raise ValueError("table must be [rotations,3] (grid_match_table)")
    out = _out_of(GridMatch, out, dev, B=B, K=int(rotations), T=2 * int(reach) + 1)
    if B == 0:
        return out
    with torch.cuda.device(dev):
        _lib.call("pof_grid_match", _ptr(ranges), _ptr(tab), *[_ptr(t) for t in gate], float(cls_thresh),
                  float(max_range), _ptr(state.grid), _ptr(state.origin), float(res), _ptr(table), int(reach),
                  int(rotations), int(min_points), int(min_score), int(min_gain), B, N, H, W, _ptr(pose), _ptr(rot),
                  _ptr(trans), *[_ptr(t) for t in out], _stream())
    return out


GridRefine = _record("GridRefine", correction=(_F64, "B", 3), score=(_F64, "B", 2), obs=(_F64, "B"), votes=(_I32, "B"),
                     count=(_I32, "B"), iters_used=(_I32, "B"), ok=(_U8, "B"), moved=(_U8, "B"))


def grid_refine_check(cap, iters, min_points, **not_negative):
    """The settings of ``grid_refine`` with a range, checked as its launcher checks them, or this raises; the keywords
    (``min_pivot``, ``max_shift``, ``max_turn``) must be >= 0.  What wraps the stage checks its settings here, before
    anything is allocated."""
    if not 1 <= int(cap) <= 32767:
        raise ValueError("cap must be in [1, 32767]")
    if not 1 <= int(iters) <= 32:
        raise ValueError("iters must be in [1, 32]")
    if int(min_points) < 0:
        raise ValueError("min_points must be >= 0")
    for name, v in not_negative.items():
        if not float(v) >= 0.0:
            raise ValueError("%s must be >= 0" % name)


def grid_refine_buffers(B, device="cuda"):
    """The eight outputs of ``grid_refine`` for B sensors, zero-filled, as its ``out=`` (allocate once, before a graph
    capture)."""
    return _zeros_of(GridRefine, device, B=B)


def grid_refine(ranges, tab, rot, trans, pose, state, *, res, instance_mask=None, num_det=None, det_cls=None,
                cls_thresh=0.5, max_range=20.0, cap=32, iters=8, min_points=50, min_pivot=1e-6, max_shift=2.0,
                max_turn=0.05, eps_shift=1e-3, eps_turn=1e-5, out=None):
    """N19: the pose of every sensor fitted to its occupancy grid below the size of a cell, one launch per batch
    (include/pof_abi.h states the rules in full).

    ranges [B,N] f32, the current scan; tab the angle table; rot [B,2,2] (or [B,4]) f32, trans [B,2] f64 and pose [B,3]
    f64 = (x, y, phi), the sensor's pose at this scan as ``pose_advance`` (and ``grid_match``) leave it, all three
    UPDATED IN PLACE when a sensor is moved.  ``state``: the ``GridMapState`` of ``grid_map_update``, read only; ``res``:
    its metres per cell.  The endpoints of the points that vote (finite, 0 < r < ``max_range``, no point of a detection
    of score >= ``cls_thresh`` when the NMS results instance_mask [B,N] i32, num_det [B] i32, det_cls [B,N] f64 are
    given, all three or none) are fitted to the grid's counts, clamped to +-``cap``, scaled to [-1, 1] and interpolated
    bilinearly between cell centres: up to ``iters`` Gauss-Newton updates of (x, y, phi), stopped early by an update
    below ``eps_shift`` cells and ``eps_turn`` radians.  The fit is ``ok`` with at least ``min_points`` voting points
    inside the grid at every evaluation and a 3 x 3 system whose pivots pass ``min_pivot`` (a corridor does not); the
    sensor is ``moved`` when the correction stays within ``max_shift`` cells and ``max_turn`` radians and the mean
    interpolated value under the scan rose.
    -> ``GridRefine``: correction [B,3] f64 = what was added to (x, y, phi), zeros without ``moved``; score [B,2] f64 =
    the mean interpolated value (before, after; after is NaN when not ``ok``); obs [B] f64, the smallest pivot over the
    largest diagonal entry; votes, count (the voting points inside the grid at the incoming pose), iters_used [B] i32;
    ok, moved [B] u8.  The same bits in every run.  ``out``: a ``GridRefine`` of preallocated tensors
    (``grid_refine_buffers``)."""
    ranges, tab, B, N, dev = _scan_input(ranges, tab)
    _pose_input(B, rot, trans, pose)
    gate = _nms_gate(instance_mask, num_det, det_cls, B, N, strict=True)
    state, H, W = _grid_state(state, B)
    grid_refine_check(cap, iters, min_points, min_pivot=min_pivot, max_shift=max_shift, max_turn=max_turn)
    out = _out_of(GridRefine, out, dev, B=B)
    if B == 0:
        return out
    with torch.cuda.device(dev):
        _lib.call("pof_grid_refine", _ptr(ranges), _ptr(tab), *[_ptr(t) for t in gate], float(cls_thresh),
                  float(max_range), _ptr(state.grid), _ptr(state.origin), float(res), int(cap), int(iters),
                  int(min_points), float(min_pivot), float(max_shift), float(max_turn), float(eps_shift),
                  float(eps_turn), B, N, H, W, _ptr(pose), _ptr(rot), _ptr(trans), *[_ptr(t) for t in out], _stream())
    return out


GridScrollState = _record("GridScrollState", persistent=dict(base=(_F64, "B", 2), offset=(_I32, "B", 2)),
                          scratch=(_I16, "B", "H", "W"))
GridScroll = _record("GridScroll", shift=(_I32, "B", 2), scrolled=(_U8, "B"))


def grid_scroll_buffers(B, device="cuda"):
    """The two outputs of ``grid_scroll`` for B sensors, zero-filled, as its ``out=`` (allocate once, before a graph
    capture)."""
    return _zeros_of(GridScroll, device, B=B)


def grid_scroll_state(B, H, W, device="cuda"):
    """What ``grid_scroll`` keeps for B sensors beside the ``GridMapState`` it scrolls: the origin of the last reset,
    the shift since then in tiles, and a workspace of the grid's size (allocate once, before a graph capture).
    -> ``GridScrollState``."""
    return _zeros_of(GridScrollState, device, B=B, H=H, W=W)


def grid_scroll_reset(scroll, state):
    """The grid of ``state`` (a ``GridMapState``) stands where it was reset to: base <- state.origin and offset <- 0, in
    place, with tensor ops on the current stream (no host sync).  Call it after any ``grid_map_reset``."""
    scroll = GridScrollState(*scroll)
    scroll.base.copy_(GridMapState(*state).origin)
    scroll.offset.zero_()
    return scroll


def grid_scroll_margin(H, W, margin=None):
    """The ``margin`` of ``grid_scroll`` for a grid of H x W cells.  None: the default, a quarter of the shorter side
    rounded down to a multiple of 64.  A given one must lie in [0, 64 floor((side / 64 - 1) / 2)] for both sides -- a
    re-centred sensor then stands outside it -- or this raises: what wraps the stage checks its setting here, before
    anything is allocated."""
    if margin is None:
        return min(int(H), int(W)) // 4 // 64 * 64
    if not 0 <= int(margin) <= 64 * ((min(int(H), int(W)) // 64 - 1) // 2):
        raise ValueError("margin must be in [0, 64 floor((side / 64 - 1) / 2)]")
    return int(margin)


def grid_scroll(trans, state, scroll, *, res, margin=None, out=None):
    """N14: the occupancy grid of every sensor follows it, two launches per batch (include/pof_abi.h states the rule in
    full).

    trans [B,2] f64, the sensor's position at this scan as ``pose_advance`` and the keyframe matchers write it.
    ``state``: the ``GridMapState`` of ``grid_map_update``, grid AND origin UPDATED IN PLACE; ``scroll``: a
    ``GridScrollState`` (``grid_scroll_state``, set by ``grid_scroll_reset``), its offset UPDATED IN PLACE; ``res``: the
    grid's metres per cell.  A sensor within ``margin`` cells of a border of its grid (None: ``grid_scroll_margin``, a
    quarter of the shorter side in whole tiles; at most 64 floor((side / 64 - 1) / 2)) has the grid shifted by whole
    tiles of 64 cells so that it stands on the middle tile again; what scrolls in is unknown (0), the origin moves with
    it, and a grid that does not scroll keeps every bit.
    -> ``GridScroll``: shift [B,2] i32 = the shift of this call in tiles (x, y), scrolled [B] u8.  The same bits in every
    run.  ``out``: a ``GridScroll`` of preallocated tensors (``grid_scroll_buffers``)."""
    trans, state, scroll, B, H, W, dev = _scroll_input(trans, state, scroll)
    out = _out_of(GridScroll, out, dev, B=B)
    if B == 0:
        return out
    with torch.cuda.device(dev):
        _lib.call("pof_grid_scroll", _ptr(trans), float(res), int(grid_scroll_margin(H, W) if margin is None else margin),
                  B, H, W, *[_ptr(t) for t in state], *[_ptr(t) for t in scroll], *[_ptr(t) for t in out], _stream())
    return out


def _scroll_input(trans, state, scroll):
    """What ``grid_scroll`` and ``grid_scroll_store`` take alike, checked -> (trans, state, scroll, B, H, W, device)."""
    if trans is None:
        raise TypeError("trans must be a tensor on the HIP device (no CPU path)")
    trans = _dev(trans, torch.float64, "trans")
    if trans.dim() != 2 or trans.shape[1] != 2:
        raise ValueError("trans must be [B,2]")
    B, dev = trans.shape[0], trans.device
    state, H, W = _grid_state(state, B)
    return trans, state, _checked(GridScrollState, scroll, "scroll", B=B, H=H, W=W), B, H, W, dev


# the store of tiles behind the window carries over from scan to scan; "S" slots, "tiles" = H / 64 * W / 64
GridStoreState = _record("GridStoreState",
                         persistent=dict(store=(_I16, "B", "S", 64, 64), store_key=(_I32, "B", "S", 2),
                                         store_stamp=(_I32, "B", "S"), clock=(_I32, "B")),
                         plan_in=(_I32, "B", "tiles"), plan_out=(_I32, "B", "tiles"))
GridScrollStore = _record("GridScrollStore", shift=(_I32, "B", 2), scrolled=(_U8, "B"), counts=(_I32, "B", 4))
GRID_STORE_MAX_SLOTS = 1024


def grid_store_slots(slots):
    """The ``slots`` setting of the tile store, in [1, 1024], or this raises: what wraps the stage checks its setting
    here, before anything is allocated."""
    if not 1 <= int(slots) <= GRID_STORE_MAX_SLOTS:
        raise ValueError("slots must be in [1, %d]" % GRID_STORE_MAX_SLOTS)
    return int(slots)


def grid_scroll_store_buffers(B, device="cuda"):
    """The three outputs of ``grid_scroll_store`` for B sensors, zero-filled, as its ``out=`` (allocate once, before a
    graph capture)."""
    return _zeros_of(GridScrollStore, device, B=B)


def grid_store_state(B, H, W, slots, device="cuda"):
    """The tile store of ``grid_scroll_store`` for B sensors with grids of H x W cells: ``slots`` tiles of 64 x 64 cells
    per sensor (8 KiB each) with their keys and stamps, the scroll clock, and the plan workspace of the launches, all
    zeros -- an empty store (allocate once, before a graph capture).  -> ``GridStoreState``."""
    H, W = grid_shape((H, W))
    return _zeros_of(GridStoreState, device, B=B, S=grid_store_slots(slots), tiles=(H // 64) * (W // 64))


def grid_store_reset(store):
    """Empties the store: store_stamp <- 0 and clock <- 0, in place, with tensor ops on the current stream (no host
    sync).  Call it with every ``grid_scroll_reset``: the keys count tiles from the origin that one sets."""
    store = GridStoreState(*store)
    store.store_stamp.zero_()
    store.clock.zero_()
    return store


def grid_scroll_store(trans, state, scroll, store, *, res, margin=None, out=None):
    """N20: ``grid_scroll`` with a store of tiles behind the window, three launches per batch (include/pof_abi.h states
    the rule in full).

    trans, ``state``, ``scroll``, ``res`` and ``margin`` are ``grid_scroll``'s, and so is all it does to them: the
    shift, the offset, the origin and the cells that stay inside.  ``store``: a ``GridStoreState``
    (``grid_store_state``), UPDATED IN PLACE.  A tile that leaves the window and is not all unknown is copied into a
    slot of the store under its world tile -- free slots first, then the slot written longest ago -- and a tile that
    scrolls in is looked up there: found, its cells come back bit for bit and its slot is released; not found, it is
    unknown (0) as in ``grid_scroll``.
    -> ``GridScrollStore``: shift [B,2] i32, scrolled [B] u8, counts [B,4] i32 = (restored, stored, evicted, dropped)
    tiles of this call.  The same bits in every run.  ``out``: a ``GridScrollStore`` of preallocated tensors
    (``grid_scroll_store_buffers``)."""
    trans, state, scroll, B, H, W, dev = _scroll_input(trans, state, scroll)
    if not isinstance(store[0], torch.Tensor) or store[0].dim() != 4:
        raise TypeError("store.store must be a [B,S,64,64] tensor on the HIP device (no CPU path)")
    S = store[0].shape[1]
    store = _checked(GridStoreState, store, "store", B=B, S=grid_store_slots(S), tiles=(H // 64) * (W // 64))
    out = _out_of(GridScrollStore, out, dev, B=B)
    if B == 0:
        return out
    with torch.cuda.device(dev):
        _lib.call("pof_grid_scroll_store", _ptr(trans), float(res),
                  int(grid_scroll_margin(H, W) if margin is None else margin), S, B, H, W, *[_ptr(t) for t in state],
                  *[_ptr(t) for t in scroll], *[_ptr(t) for t in store], *[_ptr(t) for t in out], _stream())
    return out


# the evidence of a track slot carries over from scan to scan; the classes describe one step
TrackMapState = _record("TrackMapState",
                        persistent=dict(ev_id=(_I32, "B", "M"), ev_points=(_I32, "B", "M"), ev_free=(_I32, "B", "M"),
                                        ev_occ=(_I32, "B", "M"), ev_scans=(_I32, "B", "M"), ev_start=(_F64, "B", "M", 2),
                                        ev_moved=(_U8, "B", "M")))
TrackMap = _record("TrackMap", det_occ=(_I32, "B", "N"), track_class=(_U8, "B", "M"), det_class=(_U8, "B", "N"),
                   point_class=(_U8, "B", "N"), class_count=(_I32, "B", 4))
TRACK_CLASSES = ("undecided", "free-standing", "unsupported", "background")     # the values of a class, 0..3


def track_map_state(B, max_tracks, device="cuda"):
    """The persistent state of ``track_map`` for B sensors of ``max_tracks`` slots: no evidence (allocate once, before
    a graph capture).  -> ``TrackMapState``."""
    return _zeros_of(TrackMapState, device, B=B, M=int(max_tracks))


def track_map_buffers(B, max_tracks, N, device="cuda"):
    """The five outputs of ``track_map`` for B sensors, ``max_tracks`` slots and N points, zero-filled, as its ``out=``
    (allocate once, before a graph capture)."""
    return _zeros_of(TrackMap, device, B=B, M=int(max_tracks), N=N)


def track_map_reset(state):
    """Forget the evidence of every slot, in place, with tensor ops on the current stream (no host sync)."""
    state = TrackMapState(*state)
    for t in state:
        t.zero_()
    return state


def track_map(tracks, grid_out, instance_mask, num_det, state, *, occ_thresh=17, free_pct=50, occ_pct=50,
              min_points=20, min_scans=3, travel=0.5, cap=4096, out=None):
    """N15: what the occupancy grid says about every track, one launch per batch (include/pof_abi.h states the rules
    in full).

    ``tracks``: the ``TrackState`` of this step's ``track_update``; ``grid_out``: the ``GridMapOut`` of this step's
    ``grid_map_update`` (with the NMS results); instance_mask [B,N] i32 and num_det [B] i32 as the NMS returns them; all
    read only.  ``state``: a ``TrackMapState`` (``track_map_state``), UPDATED IN PLACE: per track slot the points of
    the detections the track was matched with, how many of them lay on cells seen free (``det_free``) and on cells that
    held >= ``occ_thresh`` before the scan, the scans that added some, where the track stood when its evidence started
    and whether it has been ``travel`` metres from there since.  Beyond ``cap`` points (N <= cap <= 2^20) the three
    sums are halved.  A slot that is freed or reused starts again.  From ``min_scans`` scans and ``min_points`` points a
    track has a class: 3 background (at least ``occ_pct`` per cent of its points on occupied cells), else 1
    free-standing (it moved, or at least ``free_pct`` per cent on free cells), else 2 unsupported; 0 is undecided.
    -> ``TrackMap``: det_occ [B,N] i32, track_class [B,M] u8, det_class [B,N] u8 (the class of the track matched with
    each detection row), point_class [B,N] u8 (of the track every scan point belongs to), class_count [B,4] i32 (live
    tracks per class).  max_tracks <= 256, N <= 4096.  The same bits in every run.  ``out``: a ``TrackMap`` of
    preallocated tensors (``track_map_buffers``)."""
    tracks, grid_out = TrackState(*tracks), GridMapOut(*grid_out)
    if not isinstance(tracks.track_id, torch.Tensor) or tracks.track_id.dim() != 2 or \
            not isinstance(grid_out.point_cell, torch.Tensor) or grid_out.point_cell.dim() != 2:
        raise TypeError("tracks.track_id must be a [B,max_tracks] and grid_out.point_cell a [B,N] tensor on the HIP "
                        "device (no CPU path)")
    (B, M), N, dev = tracks.track_id.shape, grid_out.point_cell.shape[1], tracks.track_id.device
    tracks = _checked(TrackState, tracks, "tracks", B=B, M=M, N=N)
    grid_out = _checked(GridMapOut, grid_out, "grid_out", B=B, N=N)
    instance_mask = _dev(instance_mask, torch.int32, "instance_mask")
    num_det = _dev(num_det, torch.int32, "num_det")
    if tuple(instance_mask.shape) != (B, N) or tuple(num_det.shape) != (B,):
        raise ValueError("instance_mask must be [B,N] and num_det [B]")
    state = _checked(TrackMapState, state, "state", B=B, M=M)
    out = _out_of(TrackMap, out, dev, B=B, M=M, N=N)
    if B == 0:
        return out
    with torch.cuda.device(dev):
        _lib.call("pof_track_map", _ptr(instance_mask), _ptr(num_det), _ptr(grid_out.point_cell),
                  _ptr(grid_out.point_prior), _ptr(grid_out.det_points), _ptr(grid_out.det_free), _ptr(tracks.track_id),
                  _ptr(tracks.track_state), _ptr(tracks.track_det), B, N, M, *[_ptr(t) for t in state],
                  *[_ptr(t) for t in out], int(occ_thresh), int(free_pct), int(occ_pct), int(min_points),
                  int(min_scans), float(travel), int(cap), _stream())
    return out


GridCast = _record("GridCast", exp_range=(_F64, "B", "N"), exp_far=(_F64, "B", "N"), free_range=(_F64, "B", "N"),
                   exp_cell=(_I32, "B", "N"), exp_state=(_U8, "B", "N"), exp_steps=(_I32, "B", "N"),
                   point_class=(_U8, "B", "N"), det_novel=(_I32, "B", "N"), det_map=(_I32, "B", "N"),
                   det_through=(_I32, "B", "N"), class_count=(_I32, "B", 5))
CAST_STATES = ("none", "open", "edge", "wall", "outside")           # the values of exp_state, 0..4
CAST_CLASSES = ("none", "map", "novel", "through", "unknown")       # the values of point_class, 0..4


def grid_cast_buffers(B, N, device="cuda"):
    """The eleven outputs of ``grid_cast`` for B scans of N points, zero-filled, as its ``out=`` (allocate once, before
    a graph capture)."""
    return _zeros_of(GridCast, device, B=B, N=N)


def grid_cast(ranges, tab, rot, trans, state, *, res, instance_mask=None, num_det=None, det_cls=None, max_range=20.0,
              tol=None, occ_thresh=17, free_thresh=16, out=None):
    """N16: the scan the occupancy grid predicts, one ray cast per beam, two launches per batch (include/pof_abi.h
    states the rules in full).

    ranges [B,N] f32, the current scan; tab the angle table; rot [B,2,2] (or [B,4]) f32 and trans [B,2] f64, the
    sensor's pose at this scan.  ``state``: the ``GridMapState`` of ``grid_map_update``, read only, and read as it
    stands: call this in front of the scan's ``grid_map_update``, as ``point_prior`` is taken; ``res``: its metres per
    cell.  Every beam is walked from the sensor's cell through the grid, cell by cell, up to ``max_range``: the first
    cell that holds >= ``occ_thresh`` starts an occupied run, the first cell behind it that does not ends it, and the
    first cell that holds more than -``free_thresh`` is where known free space ends.  A point (finite, 0 < r <
    ``max_range``) is MAP when it lies within ``tol`` (None: ``res``) of the run, THROUGH when it lies behind it, NOVEL
    when it lies in front of the run -- or where the map has none -- with only known-free cells on the way, else
    UNKNOWN.  With the NMS results instance_mask [B,N] i32, num_det [B] i32, det_cls [B,N] f64 (all three or none) the
    classes are also counted per detection row; no score gates anything.
    -> ``GridCast``: exp_range, exp_far [B,N] f64 (where the beam enters and leaves the run, +inf without one),
    free_range [B,N] f64 (+inf when every cell was known free), exp_cell [B,N] i32 (iy W + ix of the run's first cell
    or -1), exp_state [B,N] u8 (``CAST_STATES``: 0 none, 1 open, 2 edge, 3 wall, 4 outside), exp_steps [B,N] i32,
    point_class [B,N] u8 (``CAST_CLASSES``: 0 none, 1 map, 2 novel, 3 through, 4 unknown), det_novel, det_map,
    det_through [B,N] i32 per detection row (zeros without the NMS results), class_count [B,5] i32.  N <= 4096.  The
    same bits in every run.  ``out``: a ``GridCast`` of preallocated tensors (``grid_cast_buffers``)."""
    ranges, tab, B, N, dev = _scan_input(ranges, tab)
    _pose_input(B, rot, trans)
    gate = _nms_gate(instance_mask, num_det, det_cls, B, N, strict=True)
    state, H, W = _grid_state(state, B)
    out = _out_of(GridCast, out, dev, B=B, N=N)
    if B == 0:
        return out
    with torch.cuda.device(dev):
        _lib.call("pof_grid_cast", _ptr(ranges), _ptr(tab), _ptr(rot), _ptr(trans), *[_ptr(t) for t in gate],
                  _ptr(state.grid), _ptr(state.origin), float(res), float(max_range), float(res if tol is None else tol),
                  int(occ_thresh), int(free_thresh), B, N, H, W, *[_ptr(t) for t in out], _stream())
    return out


NovelSegments = _record("NovelSegments", instance_mask=(_I32, "B", "N"), num_det=(_I32, "B"), det_xy=(_F64, "B", "N", 2),
                        det_cls=(_F64, "B", "N"), det_count=(_I32, "B", "N"), det_first=(_I32, "B", "N"),
                        det_last=(_I32, "B", "N"), det_width2=(_F64, "B", "N"), det_known=(_I32, "B", "N"),
                        seg_count=(_I32, "B", 3))


def novel_segments_buffers(B, N, device="cuda"):
    """The ten outputs of ``novel_segments`` for B scans of N points, zero-filled, as its ``out=`` (allocate once, before
    a graph capture)."""
    return _zeros_of(NovelSegments, device, B=B, N=N)


def novel_segments(ranges, tab, point_class, *, instance_mask=None, num_det=None, det_cls=None, cls_thresh=0.5,
                   jump=0.3, max_skip=2, min_points=3, max_width=1.0, out=None):
    """N17: the NOVEL points of a scan grouped into detections, one launch per batch (include/pof_abi.h states the
    rules in full).

    ranges [B,N] f32, the scan; tab the angle table; point_class [B,N] u8 as ``grid_cast`` returns it.  A beam is a
    member when its class is 2 (novel) and its range is finite and > 0.  The members are walked in beam order: one
    continues the open segment when the member before it is at most ``max_skip`` beams back and at most ``jump`` metres
    away, else it opens a new one.  A segment of fewer than ``min_points`` members is dropped, then one whose first and
    last member lie more than ``max_width`` metres apart; the kept ones are numbered in the order of their first beam.
    With the NMS results instance_mask [B,N] i32, num_det [B] i32, det_cls [B,N] f64 (all three or none) ``det_known``
    says how many members of a row belong to a detection with a score >= ``cls_thresh``.
    -> ``NovelSegments``: instance_mask [B,N] i32, num_det [B] i32, det_xy [B,N,2] f64 (the mean of the row's points in
    the sensor frame), det_cls [B,N] f64 (1.0 on a kept row) -- the four results of ``nms_predicted_center`` in the
    argument order of ``person_motion``, so ``person_motion(ranges, tab, *rec[:4], ...)`` takes them -- det_count,
    det_first, det_last [B,N] i32, det_width2 [B,N] f64, det_known [B,N] i32 (rows >= num_det[b] are zeros) and
    seg_count [B,3] i32 (segments before the filters, dropped as few, dropped as wide).  N <= 4096.  The same bits in
    every run.  ``out``: a ``NovelSegments`` of preallocated tensors (``novel_segments_buffers``)."""
    ranges, tab, B, N, dev = _scan_input(ranges, tab)
    point_class = _dev(point_class, torch.uint8, "point_class")
    if tuple(point_class.shape) != (B, N):
        raise ValueError("point_class must be [B,N]")
    gate = _nms_gate(instance_mask, num_det, det_cls, B, N, strict=True)
    out = _out_of(NovelSegments, out, dev, B=B, N=N)
    if B == 0:
        return out
    with torch.cuda.device(dev):
        _lib.call("pof_novel_segments", _ptr(ranges), _ptr(tab), _ptr(point_class), *[_ptr(t) for t in gate],
                  float(cls_thresh), float(jump), int(max_skip), int(min_points), float(max_width), B, N,
                  *[_ptr(t) for t in out], _stream())
    return out


MergedDetections = _record("MergedDetections", instance_mask=(_I32, "B", "N"), num_det=(_I32, "B"),
                           det_xy=(_F64, "B", "N", 2), det_cls=(_F64, "B", "N"), det_points=(_I32, "B", "N"),
                           det_src=(_U8, "B", "N"), det_row=(_I32, "B", "N"), b_row=(_I32, "B", "N"),
                           b_count=(_I32, "B", "N"), b_known=(_I32, "B", "N"), merge_count=(_I32, "B", 4))


def merge_detections_buffers(B, N, device="cuda"):
    """The eleven outputs of ``merge_detections`` for B scans of N points, zero-filled, as its ``out=`` (allocate once,
    before a graph capture)."""
    return _zeros_of(MergedDetections, device, B=B, N=N)


def merge_detections(b_instance_mask, b_num_det, b_det_xy, b_det_cls, *, instance_mask=None, num_det=None, det_xy=None,
                     det_cls=None, cls_thresh=0.5, absorb_pct=50, out=None):
    """N18: two detection records made one, one launch per batch (include/pof_abi.h states the rules in full).

    b_instance_mask [B,N] i32, b_num_det [B] i32, b_det_xy [B,N,2] f64, b_det_cls [B,N] f64: the secondary record, e.g.
    the first four fields of ``novel_segments``.  instance_mask, num_det, det_xy, det_cls: the primary record of the same
    shapes, as ``nms_predicted_center`` returns it, all four or none (an empty one).  A point is confident when its
    primary row has a score >= ``cls_thresh``.  A secondary row is absorbed when it has no points or at least
    ``absorb_pct`` per cent (an int in [0, 101]) of them are confident; the others are appended behind the primary rows
    in their order while there is room below N, and take their points that are not confident.  The primary rows, and the
    appended rows' centres and scores, are copied bit for bit.
    -> ``MergedDetections``: instance_mask [B,N] i32, num_det [B] i32, det_xy [B,N,2] f64, det_cls [B,N] f64 -- the
    argument order of ``person_motion``, so ``person_motion(ranges, tab, *rec[:4], ...)`` takes them -- det_points
    [B,N] i32, det_src [B,N] u8 (1 primary, 2 secondary), det_row [B,N] i32 (the row in its own record) per merged row
    (rows >= num_det[b] are zeros); b_row [B,N] i32 (the merged row, -1 absorbed, -2 dropped, -1 beyond b_num_det),
    b_count, b_known [B,N] i32 per secondary row; merge_count [B,4] i32 (primary rows, appended, absorbed, dropped).
    N <= 4096.  The same bits in every run.  ``out``: a ``MergedDetections`` of preallocated tensors
    (``merge_detections_buffers``)."""
    b_instance_mask = _dev(b_instance_mask, torch.int32, "b_instance_mask")
    if b_instance_mask.dim() != 2:
        raise ValueError("b_instance_mask must be [B,N]")
    B, N = b_instance_mask.shape
    dev = b_instance_mask.device
    sec = (b_instance_mask, _dev(b_num_det, torch.int32, "b_num_det"), _dev(b_det_xy, torch.float64, "b_det_xy"),
           _dev(b_det_cls, torch.float64, "b_det_cls"))
    if [tuple(t.shape) for t in sec[1:]] != [(B,), (B, N, 2), (B, N)]:
        raise ValueError("b_instance_mask and b_det_cls must be [B,N], b_num_det [B] and b_det_xy [B,N,2]")
    given = sum(t is not None for t in (instance_mask, num_det, det_xy, det_cls))
    if given not in (0, 4):
        raise ValueError("instance_mask, num_det, det_xy and det_cls (the primary record) come together or not at all")
    prim = _nms_results(instance_mask, num_det, det_xy, det_cls, B, N) if given else (None,) * 4
    out = _out_of(MergedDetections, out, dev, B=B, N=N)
    if B == 0:
        return out
    with torch.cuda.device(dev):
        _lib.call("pof_merge_detections", *[_ptr(t) for t in sec], *[_ptr(t) for t in prim], float(cls_thresh),
                  int(absorb_pct), B, N, *[_ptr(t) for t in out], _stream())
    return out


def flow_errors(pred, target, mask=None):
    """A12 reductions: returns (epe_sum [B], aae_sum [B] radians, count [B]) float64."""
    pred = _dev(pred, torch.float32, "pred")
    target = _dev(target, torch.float32, "target")
    if pred.shape != target.shape or pred.dim() != 3 or pred.shape[-1] != 2:
        raise ValueError("pred/target must be [B,N,2]")
    B, N = pred.shape[:2]
    if mask is not None:
        mask = _dev(mask, torch.float32, "mask")
        if tuple(mask.shape) != (B, N):
            raise ValueError("mask must be [B,N]")
    dev = pred.device
    e = torch.empty(B, dtype=torch.float64, device=dev)
    a = torch.empty(B, dtype=torch.float64, device=dev)
    c = torch.empty(B, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.call("pof_flow_errors", _ptr(pred), _ptr(target), _ptr(mask), B, N, _ptr(e), _ptr(a), _ptr(c),
                  _stream())
    return e, a, c


def band_correlation(feat1, feat2, kernel_size=3, max_displacement=5, out=None):
    """A9: [B,C,n] x2 float32 (or float16 storage, BASELINE config 5) -> [B, 2*max_displacement+1, n] float32."""
    half = isinstance(feat1, torch.Tensor) and feat1.dtype == torch.float16
    feat1 = _dev(feat1, torch.float16 if half else torch.float32, "feat1")
    feat2 = _dev(feat2, torch.float16 if half else torch.float32, "feat2")
    entry = "pof_band_correlation_f16" if half else "pof_band_correlation"
    if feat1.shape != feat2.shape or feat1.dim() != 3:
        raise ValueError("features must be two [B,C,n] tensors of equal shape")
    B, Cc, n = feat1.shape
    D = 2 * max_displacement + 1
    if out is None:
        out = torch.empty((B, D, n), dtype=torch.float32, device=feat1.device)
    with torch.cuda.device(feat1.device):
        step = 65535
        for s in range(0, B, step):
            m = min(step, B - s)
            _lib.call(entry, _ptr(feat1[s:s + m]), _ptr(feat2[s:s + m]), _ptr(out[s:s + m]),
                      m, Cc, n, int(kernel_size), int(max_displacement), _stream())
    return out


def spatial_attention(emb_x, emb_t, x, tmpl, alpha=0.5, window_size=11, out=None):
    """A10 after the embedding: emb_* [B,N,E] float32, x/tmpl [B,N,...] float32 (or float16 storage,
    BASELINE config 5) -> (out like x, band [B,N,w], prob [B,N,w])."""
    emb_x = _dev(emb_x, torch.float32, "emb_x")
    emb_t = _dev(emb_t, torch.float32, "emb_t")
    half = isinstance(x, torch.Tensor) and x.dtype == torch.float16
    x = _dev(x, torch.float16 if half else torch.float32, "x")
    tmpl = _dev(tmpl, torch.float16 if half else torch.float32, "tmpl")
    entry = "pof_spatial_attention_f16" if half else "pof_spatial_attention"
    if emb_x.shape != emb_t.shape or emb_x.dim() != 3 or x.shape != tmpl.shape:
        raise ValueError("shape mismatch")
    B, N, E = emb_x.shape
    if x.shape[0] != B or x.shape[1] != N:
        raise ValueError("x must be [B,N,...]")
    F = x.numel() // (B * N)
    W = 2 * int(window_size / 2) + 1
    dev = x.device
    band = torch.empty((B, N, W), dtype=torch.float32, device=dev)
    prob = torch.empty((B, N, W), dtype=torch.float32, device=dev)
    if out is None:
        out = torch.empty_like(x)
    with torch.cuda.device(dev):
        step = 65535
        for s in range(0, B, step):
            m = min(step, B - s)
            _lib.call(entry, _ptr(emb_x[s:s + m]), _ptr(emb_t[s:s + m]), _ptr(x[s:s + m]),
                      _ptr(tmpl[s:s + m]), m, N, E, F, int(window_size), float(alpha), _ptr(band[s:s + m]),
                      _ptr(prob[s:s + m]), _ptr(out[s:s + m]), _stream())
    return out, band, prob


def spatial_attention_plan(B, N, F):
    """Host-only: points per lane segment of one call on B <= 65535 scans -> (forward_segment, backward_segment):
    the merge walk of spatial_attention (and of the two-pass backward), the fused backward walk.  No device work."""
    fwd, bwd = C.c_int(0), C.c_int(0)
    _lib.call("pof_spatial_attention_plan", int(B), int(N), int(F), C.byref(fwd), C.byref(bwd))
    return fwd.value, bwd.value


def attn_embed(x, tmpl, weight, bias, negative_slope=0.1):
    """A10, the gate's embedding on the folded inference route: x [R, K] (or [..., K]-shaped rows flattened by the
    caller) float32 or float16 storage, tmpl like x or None, weight [E, K] / bias [E] float32 (Conv1d + BatchNorm folded,
    ``_SpatialAttention.fold_for_inference``) -> (emb_x, emb_t | None) float32 [R, E] = LeakyReLU(rows @ weight.T + bias),
    both sources in one launch.  K % 8 == 0, E in 32, 64, .. 256, R >= 1.  One documented summation order
    (include/pof_abi.h): a row's bits do not depend on R, on the slot or on the storage type."""
    half = isinstance(x, torch.Tensor) and x.dtype == torch.float16
    act = torch.float16 if half else torch.float32
    x = _dev(x, act, "x")
    if tmpl is not None:
        tmpl = _dev(tmpl, act, "tmpl")
    weight = _dev(weight, torch.float32, "weight")
    bias = _dev(bias, torch.float32, "bias")
    if x.dim() != 2 or weight.dim() != 2 or weight.shape[1] != x.shape[1]:
        raise ValueError("x must be [R, K] and weight [E, K]")
    if tmpl is not None and tmpl.shape != x.shape:
        raise ValueError("tmpl must have x's shape")
    R, K = x.shape
    E = weight.shape[0]
    if bias.numel() != E:
        raise ValueError("bias must have E entries")
    if R < 1 or K % 8 or E % 32 or not 32 <= E <= 256:
        raise ValueError("attn_embed: needs R >= 1, K %% 8 == 0 and E in 32, 64, .. 256 (R=%d K=%d E=%d)" % (R, K, E))
    x = _aligned16(x)                # 16-byte operand rows: views at an offset go through a copy
    tmpl = None if tmpl is None else _aligned16(tmpl)
    weight = _aligned16(weight)
    emb_x = torch.empty((R, E), dtype=torch.float32, device=x.device)
    emb_t = None if tmpl is None else torch.empty((R, E), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.call("pof_attn_embed_f16" if half else "pof_attn_embed", _ptr(x), _ptr(tmpl), R, K, E, _ptr(weight),
                  _ptr(bias), float(negative_slope), _ptr(emb_x), _ptr(emb_t), _stream())
    return emb_x, emb_t


def attn_embed_plan(R, K, E):
    """Host-only: the kernel form attn_embed launches for R rows per source (0: four waves split K and meet in LDS,
    1: one wave carries the four chains of 64 rows).  No device work."""
    form = C.c_int(-1)
    _lib.call("pof_attn_embed_plan", int(R), int(K), int(E), C.byref(form))
    return form.value


def band_correlation_backward(feat1, feat2, g_out, kernel_size=3, max_displacement=5):
    """Gradients of band_correlation wrt feat1 / feat2."""
    feat1 = _dev(feat1, torch.float32, "feat1")
    feat2 = _dev(feat2, torch.float32, "feat2")
    g_out = _dev(g_out, torch.float32, "g_out")
    B, Cc, n = feat1.shape
    if tuple(g_out.shape) != (B, 2 * max_displacement + 1, n):
        raise ValueError("g_out must be [B, 2*max_displacement+1, n]")
    d1, d2 = torch.empty_like(feat1), torch.empty_like(feat2)
    with torch.cuda.device(feat1.device):
        for s in range(0, B, 65535):
            m = min(65535, B - s)
            _lib.call("pof_band_correlation_backward", _ptr(feat1[s:s + m]), _ptr(feat2[s:s + m]),
                      _ptr(g_out[s:s + m]), _ptr(d1[s:s + m]), _ptr(d2[s:s + m]), m, Cc, n, int(kernel_size),
                      int(max_displacement), _stream())
    return d1, d2


def spatial_attention_backward(emb_x, emb_t, tmpl, prob, g_out, g_band, alpha, window_size, fused=True):
    """Gradients of spatial_attention: -> (d_emb_x, d_emb_t, d_x, d_tmpl).  ``fused``: one walk over g and tmpl
    (pof_spatial_attention_backward_fused); False: the two-pass form (band product on the MFMA, transposed merge)."""
    emb_x = _dev(emb_x, torch.float32, "emb_x")
    emb_t = _dev(emb_t, torch.float32, "emb_t")
    tmpl = _dev(tmpl, torch.float32, "tmpl")
    prob = _dev(prob, torch.float32, "prob")
    g_out = _dev(g_out, torch.float32, "g_out")
    if g_band is not None:
        g_band = _dev(g_band, torch.float32, "g_band")
    B, N, E = emb_x.shape
    F = tmpl.numel() // (B * N)
    dev = tmpl.device
    dsim = torch.empty_like(prob)
    dex, det = torch.empty_like(emb_x), torch.empty_like(emb_t)
    dx, dt = torch.empty_like(tmpl), torch.empty_like(tmpl)
    with torch.cuda.device(dev):
        for s in range(0, B, 65535):
            m = min(65535, B - s)
            args = (_ptr(emb_x[s:s + m]), _ptr(emb_t[s:s + m]), _ptr(tmpl[s:s + m]), _ptr(prob[s:s + m]),
                    _ptr(g_out[s:s + m]), _ptr(g_band[s:s + m]) if g_band is not None else None, m, N, E, F,
                    int(window_size), float(alpha), _ptr(dsim[s:s + m]), _ptr(dex[s:s + m]), _ptr(det[s:s + m]),
                    _ptr(dx[s:s + m]), _ptr(dt[s:s + m]))
            if fused:
                nbytes = int(_lib.load().pof_spatial_attention_backward_workspace_bytes(m, N, F, int(window_size)))
                ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)
                _lib.call("pof_spatial_attention_backward_fused", *args, _ptr(ws), nbytes, _stream())
            else:
                _lib.call("pof_spatial_attention_backward", *args, _stream())
    return dex, det, dx, dt


def segment_features(ranges, tab, jump_dist=0.5, max_seg=None):
    """A13: ranges [B,N] float32 -> (seg_id [B,N] int32, num_seg [B] int32, feat [B,max_seg,16] f64)."""
    ranges = _dev(ranges, torch.float32, "ranges")
    B, N = ranges.shape
    max_seg = N if max_seg is None else int(max_seg)
    dev = ranges.device
    seg_id = torch.empty((B, N), dtype=torch.int32, device=dev)
    num = torch.empty(B, dtype=torch.int32, device=dev)
    feat = torch.full((B, max_seg, 16), float("nan"), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.call("pof_segment_features", _ptr(ranges), _ptr(tab), B, N, float(jump_dist), max_seg,
                  _ptr(seg_id), _ptr(num), _ptr(feat), _stream())
    return seg_id, num, feat


def segment_features_reference(ranges, tab, next_ranges=None, odom_dt=None, wp_offsets=None, wp_xy=None,
                               radius_wp=0.5, jump_dist=0.5, max_seg=None, want_plain=False):
    """A13 in the reference's own form (compute_feature, adaboost_person_det.py:102-210): ranges [B,N] float32
    -> (seg_id [B,N], num_seg [B], num_kept [B], ref_feat [B,max_seg,15] float64[, feat [B,max_seg,16]]).
    next_ranges [B,N] float32 and odom_dt [B] float64 feed the mean-speed column, the annotation CSR
    (wp_offsets [B+1] int32, wp_xy [W,2] float64) the labels."""
    ranges = _dev(ranges, torch.float32, "ranges")
    B, N = ranges.shape
    if next_ranges is not None:
        next_ranges = _dev(next_ranges, torch.float32, "next_ranges")
        if next_ranges.shape != ranges.shape:
            raise ValueError("next_ranges must have the shape of ranges")
    if odom_dt is not None:
        odom_dt = _dev(odom_dt, torch.float64, "odom_dt")
        if odom_dt.numel() != B:
            raise ValueError("odom_dt must be [B]")
    if wp_offsets is not None:
        wp_offsets = _dev(wp_offsets, torch.int32, "wp_offsets")
        wp_xy = _dev(wp_xy, torch.float64, "wp_xy")
        if wp_offsets.numel() != B + 1 or wp_xy.dim() != 2 or wp_xy.shape[1] != 2:
            raise ValueError("annotations must be CSR: wp_offsets [B+1], wp_xy [W,2]")
    max_seg = N if max_seg is None else int(max_seg)
    dev = ranges.device
    seg_id = torch.empty((B, N), dtype=torch.int32, device=dev)
    num = torch.empty(B, dtype=torch.int32, device=dev)
    kept = torch.empty(B, dtype=torch.int32, device=dev)
    ref = torch.full((B, max_seg, 15), float("nan"), dtype=torch.float64, device=dev)
    feat = torch.full((B, max_seg, 16), float("nan"), dtype=torch.float64, device=dev) if want_plain else None
    with torch.cuda.device(dev):
        _lib.call("pof_segment_features_ex", _ptr(ranges), _ptr(next_ranges), _ptr(tab), B, N, float(jump_dist),
                  _ptr(odom_dt), _ptr(wp_offsets), _ptr(wp_xy), float(radius_wp), max_seg, _ptr(seg_id), _ptr(num),
                  _ptr(kept), _ptr(feat), _ptr(ref), _stream())
    return (seg_id, num, kept, ref, feat) if want_plain else (seg_id, num, kept, ref)


_PERM_3D = [0, 1, 3, 4, 6, 2, 5]


def rotate_iou(boxes, query_boxes, criterion=-1, is_3d=False, n_valid=None, k_valid=None):
    """A16: boxes [N,s] / [G,N,s], query [K,s] / [G,K,s] float32 device tensors in the
    REFERENCE column order (3-D: x,y,z,l,w,h,rot) -> iou [N,K] / [G,N,K] float32."""
    if boxes.dim() == 2:
        return rotate_iou(boxes[None], query_boxes[None], criterion, is_3d)[0]
    s = 7 if is_3d else 5
    if boxes.shape[-1] != s or query_boxes.shape[-1] != s or boxes.shape[0] != query_boxes.shape[0]:
        raise ValueError("boxes must be [G,N,%d] and query [G,K,%d]" % (s, s))
    b = boxes.to(torch.float32)
    q = query_boxes.to(torch.float32)
    if is_3d:
        b, q = b[..., _PERM_3D], q[..., _PERM_3D]
    b = _dev(b.contiguous(), torch.float32, "boxes")
    q = _dev(q.contiguous(), torch.float32, "query_boxes")
    G, N, K = b.shape[0], b.shape[1], q.shape[1]
    out = torch.zeros((G, N, K), dtype=torch.float32, device=b.device)
    if n_valid is not None:
        n_valid = _dev(n_valid, torch.int32, "n_valid")
    if k_valid is not None:
        k_valid = _dev(k_valid, torch.int32, "k_valid")
    with torch.cuda.device(b.device):
        _lib.call("pof_rotate_iou", _ptr(b), _ptr(q), _ptr(out), G, N, K, _ptr(n_valid), _ptr(k_valid),
                  int(criterion), int(bool(is_3d)), _stream())
    return out


def gather_windows(scans_all, seq_first, scan_idx, num_scans, distance=5, stride=1, out=None):
    """N1: scans_all [S,N] f32, seq_first / scan_idx [B] int32 -> (windows [B,num_scans+1,N],
    row_cur [B], row_prev [B])."""
    scans_all = _dev(scans_all, torch.float32, "scans_all")
    seq_first = _dev(seq_first, torch.int32, "seq_first")
    scan_idx = _dev(scan_idx, torch.int32, "scan_idx")
    B, N = scan_idx.shape[0], scans_all.shape[1]
    dev = scans_all.device
    if out is None:
        out = torch.empty((B, num_scans + 1, N), dtype=torch.float32, device=dev)
    row_cur = torch.empty(B, dtype=torch.int32, device=dev)
    row_prev = torch.empty(B, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        for s in range(0, B, 65535):
            m = min(65535, B - s)
            _lib.call("pof_gather_windows", _ptr(scans_all), _ptr(seq_first[s:s + m]), _ptr(scan_idx[s:s + m]), m,
                      int(num_scans), int(distance), int(stride), N, _ptr(out[s:s + m]), _ptr(row_cur[s:s + m]),
                      _ptr(row_prev[s:s + m]), _stream())
    return out, row_cur, row_prev


def associate_odometry(scans_t, odoms_t, odoms, odom_lo, odom_hi, row_cur, row_prev):
    """N1: time association -> (odom0 [B,3] f64, odom1 [B,3] f64, idx0 [B], idx1 [B])."""
    scans_t = _dev(scans_t, torch.float32, "scans_t")
    odoms_t = _dev(odoms_t, torch.float32, "odoms_t")
    odoms = _dev(odoms, torch.float32, "odoms")
    B = row_cur.shape[0]
    dev = scans_t.device
    o0 = torch.empty((B, 3), dtype=torch.float64, device=dev)
    o1 = torch.empty((B, 3), dtype=torch.float64, device=dev)
    i0 = torch.empty(B, dtype=torch.int32, device=dev)
    i1 = torch.empty(B, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.call("pof_associate_odometry", _ptr(scans_t), _ptr(odoms_t), _ptr(odoms),
                  _ptr(_dev(odom_lo, torch.int32, "odom_lo")), _ptr(_dev(odom_hi, torch.int32, "odom_hi")),
                  _ptr(_dev(row_cur, torch.int32, "row_cur")), _ptr(_dev(row_prev, torch.int32, "row_prev")), B,
                  _ptr(o0), _ptr(o1), _ptr(i0), _ptr(i1), _stream())
    return o0, o1, i0, i1
