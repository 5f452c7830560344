"""Streaming DR-SPAAM inference as one hipGraph replay per scan.

The reference's deployment mode is ``SpatialDROW.forward(x, testing=True, fea_template=...)``
(src/depracted/model/dr_spaam.py:243-262): every new scan is cut out, run through the first two trunk
blocks, fused with the running template by the attention gate and classified; the fused template is fed
back on the next call: ~30 kernel launches per scan.  ``StreamingDetector`` keeps the scan, the template and
the outputs in fixed device buffers, captures the steady-state step once and replays it, so the host thread
issues one graph launch per scan instead of thirty kernel launches.  Measured on MI355X
(tools/bench_stream.py): the replay takes 0.57-0.60 ms per scan at one sensor and 2.11 ms at eight; the eager
step is host-bound at one sensor and took 0.60 to 2.35 ms on different boxes.  Outputs are bit-identical to the eager step.
A model fused with ``embed="hip"`` has its gate embedding as one HIP node for the scan and the template, and may keep
float16 storage (float16 cutout and template).
"""
import torch

from . import ops

_DEFAULT_CUTOUT = dict(fixed=True, centered=True, window_width=1.0, window_depth=0.5, num_cutout_pts=56,
                       padding_val=29.99, area_mode=True)


class StreamingDetector:
    """``det = StreamingDetector(model)``; ``pred_cls, pred_reg = det(scan)`` per incoming scan.

    model: an eval-mode ``SpatialDROW`` on the GPU (``fuse_for_inference()`` is applied unless the model is fused
    already; a model fused with ``storage=torch.float16, embed="hip"`` streams with a float16 cutout and a float16
    template, the outputs stay float32; float16 storage with the library embedding is refused).  scan: [N] or [B, N]
    ranges (B independent sensors advance in lock-step).  The returned tensors are the detector's fixed output
    buffers -- valid until the next call; ``.clone()`` to keep them.  ``feat_fused`` (the window similarities
    of the last step, input of the flow head) and ``template`` are attributes.  ``reset()`` forgets the
    template, as at the start of a sequence.  ``graph=False`` runs the same step eagerly (reference for
    tests and timing).  With ``nms_min_dist`` (one-logit models) the greedy centre NMS of
    ``utils.nms_predicted_center`` runs inside the same step and ``detections()`` returns its result."""

    def __init__(self, model, num_pts=450, batch=1, angle_inc=None, cutout_kwargs=None, graph=True, device="cuda",
                 nms_min_dist=None):
        if not torch.cuda.is_available():
            raise RuntimeError("StreamingDetector needs the GPU (no CPU path)")
        self._refuse_float16(model)
        self.model = model.to(device).eval()
        # The captured graph bakes in the addresses of the folded trunk parameters (model._fused).  The detector
        # therefore (i) does not re-fuse a model that is already fused -- that would free the tensors another
        # detector's graph still replays from -- and (ii) keeps its own reference to the set it captured, so the
        # memory outlives a later fuse_for_inference() / train() of the model; _ensure_fused() notices such a
        # change before every step and drops the stale graph.
        if getattr(self.model, "_fused", None) is None:
            self.model.fuse_for_inference()
        self._fused_ref = self.model._fused
        self._route = self._fuse_route()
        self.kw = dict(_DEFAULT_CUTOUT if cutout_kwargs is None else cutout_kwargs)
        self.B, self.N = int(batch), int(num_pts)
        dev = next(self.model.parameters()).device
        self.tab = ops.phi_table(num_pts=self.N, device=dev) if angle_inc is None \
            else ops.phi_table(angle_inc, self.N, device=dev)
        self._scan = torch.zeros((self.B, 1, self.N), dtype=torch.float32, device=dev)
        # the cutout's per-sample workspace is the detector's, allocated before any capture: the captured step
        # then holds no allocation that is made and dropped inside the capture
        self._cut_ws = torch.zeros(max(self.B, 1), dtype=torch.int32, device=dev)
        self._use_graph = bool(graph)
        self._nms = None if nms_min_dist is None else float(nms_min_dist)
        self._dets = None
        self._graph = None
        self.template = None            # fixed buffer once the first scan has been seen
        self._have_template = False
        self.feat_fused = self.pred_cls = self.pred_reg = None

    @staticmethod
    def _refuse_float16(model):
        """Float16 storage streams only with the HIP embedding (fuse_for_inference(storage=float16, embed="hip")):
        the library embedding needs float32 rows, i.e. a widened copy of the scan's features and of the template per
        step."""
        if getattr(model, "_fused", None) is not None and getattr(model, "_storage", torch.float32) != torch.float32 \
                and getattr(model, "_embed_route", "library") != "hip":
            raise ValueError("StreamingDetector keeps float32 storage: the model was fused with storage=%s -- "
                             "call model.fuse_for_inference() (float32) first" % model._storage)

    def _fuse_route(self):
        return (getattr(self.model, "_storage", torch.float32), getattr(self.model, "_embed_route", "library"))

    def reset(self):
        self._have_template = False

    def _ensure_fused(self):
        """The model was re-fused (new checkpoint) or left eval mode since the last step: fuse again if needed
        and forget the graph captured on the old parameter tensors."""
        if self.model.training:
            self.model.eval()
        if getattr(self.model, "_fused", None) is None:
            self.model.fuse_for_inference()
        self._refuse_float16(self.model)
        if self.model._fused is not self._fused_ref or self._fuse_route() != self._route:
            if self._fuse_route()[0] != self._route[0] and self.template is not None:
                # another storage type: the running template goes on in that type (a new buffer; the graph is dropped)
                self.template = self.template.to(self._fuse_route()[0])
            self._fused_ref = self.model._fused
            self._route = self._fuse_route()
            self._graph = None

    # one step on the static buffers; `first` = no template yet
    def _step(self, first):
        x = ops.cutout(self._scan, self.tab, workspace=self._cut_ws, out_dtype=self._route[0], **self.kw)
        with torch.no_grad():
            cls, reg, tmpl, fused = self.model(x, testing=True, fea_template=None if first else self.template)
            if self._nms is not None:
                if cls.shape[-1] != 1:
                    raise ValueError("nms_min_dist needs a one-logit (pedestrian_only) model")
                conf = torch.sigmoid(cls[..., 0]).double().contiguous()
                self._dets = ops.nms_predicted_center(self._scan[:, 0], self.tab, conf, reg.double().contiguous(), self._nms)
        return cls, reg, tmpl, fused

    def _store_template(self, tmpl):
        if self.template is None:
            self.template = tmpl.clone()              # allocated once: the captured graph holds its address
        else:
            self.template.copy_(tmpl)

    def _capture(self):
        side = torch.cuda.Stream(device=self._scan.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                 # warm-up off the capture: library handles, lazy inits
            for _ in range(2):
                self._step(False)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            cls, reg, tmpl, fused = self._step(False)
            self.template.copy_(tmpl)                 # feed the fused template back in place
        self._graph, self._out, self._graph_dets = g, (cls, reg, fused), self._dets

    def __call__(self, scan):
        scan = torch.as_tensor(scan, dtype=torch.float32)
        self._ensure_fused()
        self._scan.copy_(scan.reshape(self.B, 1, self.N), non_blocking=True)
        if not self._have_template:                   # first scan of a sequence: eager, template = its own features
            cls, reg, tmpl, fused = self._step(True)
            self._store_template(tmpl)
            self._have_template = True
        elif not self._use_graph:
            cls, reg, tmpl, fused = self._step(False)
            self._store_template(tmpl)
        else:
            if self._graph is None:
                self._capture()                       # warm-up steps read the template, nothing writes it
            self._graph.replay()
            cls, reg, fused = self._out
            self._dets = self._graph_dets
        self.pred_cls, self.pred_reg, self.feat_fused = cls, reg, fused
        return cls, reg

    def detections(self):
        """-> list (one entry per sensor) of (xy [M, 2], confidence [M]) NumPy arrays and the instance masks [B, N]
        of the last step (needs ``nms_min_dist``).  Reads the counts back, i.e. synchronises."""
        if self._dets is None:
            raise RuntimeError("construct the detector with nms_min_dist and feed it a scan first")
        xy, conf, num, inst = self._dets
        counts = num.cpu().numpy()
        return [(xy[b, :m].cpu().numpy(), conf[b, :m].cpu().numpy()) for b, m in enumerate(counts)], inst.cpu().numpy()
