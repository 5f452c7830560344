#!/usr/bin/env python3
"""Generate tests/golden/*.npz by running the REFERENCE itself (build container only).

The reference (/root/reference) is imported read-only with harness-side stubs for
the non-arithmetic modules this image lacks (cv2, numba, tensorboardX, lzf,
wandb) and the numpy aliases removed after 1.24 (np.int / np.float).  Nothing of
the reference is copied: only seeded inputs and the outputs it produced are
written, as compressed .npz data fixtures.

    python tools/gen_golden.py            # rewrites tests/golden/

The fixtures travel to the GPU box; the reference never does.
"""
import os
import sys
import types

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("POF_REFERENCE", "/root/reference")
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, REPO)


def _install_stubs():
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    stub("cv2")
    stub("tensorboardX", SummaryWriter=object)
    stub("lzf")
    stub("wandb")
    stub("tensorboard")
    stub("torch.utils.tensorboard", SummaryWriter=object)
    nb, cu = stub("numba"), stub("numba.cuda")

    def jit(*a, **k):
        if len(a) == 1 and callable(a[0]) and not k:
            return a[0]
        return lambda f: f

    nb.jit = cu.jit = jit
    nb.cuda = cu
    # the device functions of src/utils/rotate_iou.py are plain Python once these exist
    nb.float32 = np.float32
    cu.local = types.SimpleNamespace(array=lambda shape, dtype: np.zeros(shape, dtype=dtype))
    np.int = int
    np.float = float
    torch.Tensor.cuda = lambda s, *a, **k: s
    sys.path.insert(0, REF)


def gen_rotate_iou():
    """A16: the reference's own device functions (src/utils/rotate_iou.py:20-294) run as plain
    Python (numba.cuda.jit is a pass-through, cuda.local.array -> np.zeros) on random rotated boxes,
    with the host wrapper's float32 cast and 3-D column permutation (:378-384) and the kernel's
    argument order (query box first, :346-357)."""
    import src.utils.rotate_iou as rot
    rng = np.random.default_rng(1601)
    g = {}
    perm = [0, 1, 3, 4, 6, 2, 5]

    def boxes2d(n, spread):
        return np.stack([rng.uniform(-spread, spread, n), rng.uniform(-spread, spread, n),
                         rng.uniform(0.2, 2.0, n), rng.uniform(0.2, 2.0, n),
                         rng.uniform(-np.pi, np.pi, n)], axis=1)

    def boxes3d(n, spread):
        b = boxes2d(n, spread)                       # x y l w rot -> x y z l w h rot
        return np.stack([b[:, 0], b[:, 1], rng.uniform(-0.5, 0.5, n), b[:, 2], b[:, 3],
                         rng.uniform(0.5, 2.0, n), b[:, 4]], axis=1)

    with np.errstate(all="ignore"):
        for tag, is_3d, mk in (("2d", False, boxes2d), ("3d", True, boxes3d)):
            for crit in (-1, 0, 1, 2):
                N, K = 12, 10
                bx, qx = mk(N, 1.0), mk(K, 1.0)
                # special pairs: identical, concentric with another angle, far apart, touching edge
                qx[0] = bx[0]
                qx[1] = bx[1]; qx[1][-1] += 0.7
                qx[2][:2] = bx[2][:2] + 50.0
                b32, q32 = bx.astype(np.float32), qx.astype(np.float32)
                if is_3d:
                    b32, q32 = b32[:, perm], q32[:, perm]
                fn = rot.devRotateIoU3dEval if is_3d else rot.devRotateIoU2dEval
                out = np.zeros((N, K), dtype=np.float32)
                for i in range(N):
                    for k in range(K):
                        out[i, k] = fn(q32[k].copy(), b32[i].copy(), crit)
                key = "%s_c%d" % (tag, crit)
                g[key + "_boxes"], g[key + "_query"], g[key + "_iou"] = bx, qx, out
    np.savez_compressed(os.path.join(OUT, "rotate_iou.npz"), **g)
    print("rotate_iou.npz:", {k: v.shape for k, v in g.items() if k.endswith("_iou")})


class _FloorRecorder:
    """Stands in for the `np` name inside src.utils.utils while scans_to_cutout runs: every attribute
    is numpy's, `floor` additionally keeps its result, so that the reference's *internal* inds_ct_low
    (utils.py:292: clip(floor(inds_ct), 0, N-1)) can be stored next to its output."""

    def __init__(self):
        self.floors = []

    def __getattr__(self, name):
        return getattr(np, name)

    def floor(self, x):
        r = np.floor(x)
        self.floors.append(r)
        return r


def _reference_cutout_with_indices(u, scans, phi, **kw):
    rec = _FloorRecorder()
    u.np = rec
    try:
        out = u.scans_to_cutout(scans, phi, **kw)
    finally:
        u.np = np
    assert len(rec.floors) == 1
    lo = np.clip(rec.floors[0], 0, scans.shape[1] - 1).astype(np.int16)      # (P, T, N/stride)
    return out, lo


def gen_cutout_indices():
    """The reference's own inds_ct_low for every fixture of cutout.npz (same seeds) and for the dense
    config-5 window of cutout_dense.npz (every 4th point)."""
    import src.utils.utils as u
    from planar_optical_flow_amd import synth
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from cases import CUTOUT_CASES
    gold = np.load(os.path.join(OUT, "cutout.npz"))
    g = {}
    for name, (inc, n, kw) in CUTOUT_CASES.items():
        scans = gold[name + "_scans"]
        ph = u.get_laser_phi(np.radians(inc), n)
        los = []
        for b in range(len(scans)):
            out, lo = _reference_cutout_with_indices(u, scans[b], ph, **kw)
            assert np.array_equal(out, gold[name + "_out"][b]), name
            los.append(lo)
        g[name + "_lo"] = np.array(los)
    dense = np.load(os.path.join(OUT, "cutout_dense.npz"))
    ph = u.get_laser_phi(np.radians(0.1), 3600)
    out, lo = _reference_cutout_with_indices(u, dense["scans"][0], ph, **CUTOUT_CASES["dense3600"][2])
    assert np.array_equal(out[::4], dense["out"][0])
    g["dense_t11_lo"] = lo[None, :, :, ::4]
    np.savez_compressed(os.path.join(OUT, "cutout_indices.npz"), **g)
    print("cutout_indices.npz:", {k: v.shape for k, v in g.items()})


def gen_cutout_dense():
    """BASELINE config 5 at size: one 3600-point, 11-scan window through the reference's cutout."""
    import src.utils.utils as u
    from planar_optical_flow_amd import synth
    kw = dict(fixed=True, centered=True, window_width=1.0, window_depth=0.5, num_cutout_pts=56,
              padding_val=29.99, area_mode=True)
    sb = synth.make_batch(seed=105, B=1, T=11, N=3600, angle_inc=np.radians(0.1))
    ph = u.get_laser_phi(np.radians(0.1), 3600)
    out = u.scans_to_cutout(sb.scans[0], ph, **kw)
    # (3600, 11, 56) float32 = 8.9 MB raw: every 4th point is stored (points are independent given
    # the call-wide s_area, which the full call above fixed)
    np.savez_compressed(os.path.join(OUT, "cutout_dense.npz"), scans=sb.scans, point_stride=np.array(4),
                        out=out[None, ::4])
    print("cutout_dense.npz:", out.shape, out.dtype)


def gen_gradients():
    """Backward passes of the REFERENCE under torch autograd on the CPU (round 3): upstream gradients are seeded,
    the fixture holds inputs, upstream gradients and the gradients the reference's own graph produces.
      A9   Prototype._fusion                 d feat1, d feat2                     prototype.py:118-156
      A10  _SpatialAttention.forward         d x, d x_template, d emb (both conv outputs), d conv weight / bias /
                                             BatchNorm affine                     dr_spaam.py:163-217
      N2   SpatialDROW train-mode step       loss + every parameter's gradient as (sum, abs-sum) and a few whole
           (model_fn_obj_det)                tensors, in float32 (the reference as it runs) and with its
                                             modules in float64 (the yardstick)   dr_spaam.py:41-121, 220-277
           Prototype train-mode step         loss (EPE) + gradient summaries      prototype.py:57-109
    """
    from src.depracted.model import prototype as proto
    from src.depracted.model import dr_spaam as spaam
    from src.utils import eval_utils
    g = {}
    # ---- A9
    torch.manual_seed(141)
    for tag, shape, kw in (("corr", (2, 256, 57), {}), ("corr_s", (3, 16, 23), {"kernel_size": 3, "max_displacement": 3})):
        f1 = torch.randn(*shape, requires_grad=True)
        f2 = torch.randn(*shape, requires_grad=True)
        out = proto.Prototype._fusion(None, f1, f2, **kw)
        up = torch.randn_like(out)
        d1, d2 = torch.autograd.grad(out, [f1, f2], up)
        g[tag + "_f1"], g[tag + "_f2"], g[tag + "_up"] = f1.detach().numpy(), f2.detach().numpy(), up.numpy()
        g[tag + "_out"], g[tag + "_d1"], g[tag + "_d2"] = out.detach().numpy(), d1.numpy(), d2.numpy()
    # ---- A10 (eval-mode BatchNorm in the embedding: the gate's arithmetic without batch coupling)
    for tag, seed, (B, n_cut, n_ch, n_pts), alpha, w in (("attn", 151, (2, 40, 32, 14), 0.5, 11),
                                                         ("attn_w7", 152, (1, 19, 8, 5), 0.3, 7)):
        torch.manual_seed(seed)
        att = spaam._SpatialAttention(n_pts=n_pts, n_channel=n_ch, alpha=alpha, window_size=w)
        att.eval()
        with torch.no_grad():
            att.conv[1].running_mean.normal_(0, 0.1)
            att.conv[1].running_var.uniform_(0.5, 1.5)
        x = torch.randn(B, n_cut, n_ch, n_pts, requires_grad=True)
        t = torch.randn(B, n_cut, n_ch, n_pts, requires_grad=True)
        embs = []

        def keep(_m, _i, o):            # the embedding convolution runs twice: x, then the template
            o.retain_grad()
            embs.append(o)

        hook = att.conv.register_forward_hook(keep)
        out, band = att(x, t)
        hook.remove()
        up_out, up_band = torch.randn_like(out), torch.randn_like(band)
        torch.autograd.backward([out, band], [up_out, up_band])
        for k, v in att.state_dict().items():
            g[tag + "_sd_" + k.replace(".", "_")] = v.numpy()
        g[tag + "_x"], g[tag + "_t"] = x.detach().numpy(), t.detach().numpy()
        g[tag + "_out"], g[tag + "_band"] = out.detach().numpy(), band.detach().numpy()
        g[tag + "_up_out"], g[tag + "_up_band"] = up_out.numpy(), up_band.numpy()
        g[tag + "_dx"], g[tag + "_dt"] = x.grad.numpy(), t.grad.numpy()
        g[tag + "_emb_x"], g[tag + "_emb_t"] = embs[0].detach().numpy(), embs[1].detach().numpy()
        g[tag + "_demb_x"], g[tag + "_demb_t"] = embs[0].grad.numpy(), embs[1].grad.numpy()
        for k, p in att.named_parameters():
            g[tag + "_dp_" + k.replace(".", "_")] = p.grad.numpy()
    # ---- N2: one SpatialDROW training step (BatchNorm with batch statistics, the reference's own loss adapter)
    torch.manual_seed(3)
    mref = spaam.SpatialDROW(num_scans=5, num_pts=56, alpha=0.5, window_size=11, pedestrian_only=True)
    mref.train()
    xin = torch.randn(2, 30, 5, 56) * 0.5
    rs = np.random.default_rng(23)
    tc = (rs.uniform(size=(2, 30)) < 0.3).astype(np.int64)
    tr = rs.normal(size=(2, 30, 2)).astype(np.float32)
    loss, tb, _ = eval_utils.model_fn_obj_det(mref, {"input": xin.numpy(), "target_flow_cls": tc, "target_flow_reg": tr})
    loss.backward()
    names = [k for k, _ in mref.named_parameters()]
    g["sd_x"], g["sd_cls"], g["sd_reg"] = xin.numpy(), tc, tr
    g["sd_loss"] = np.array([float(loss.detach()), tb["cls_loss"], tb["reg_loss"]])
    g["sd_names"] = np.array(names)
    g["sd_gsum"] = np.array([float(p.grad.double().sum()) for _, p in mref.named_parameters()])
    g["sd_gabs"] = np.array([float(p.grad.double().abs().sum()) for _, p in mref.named_parameters()])
    whole = ["conv_block_1.0.0.weight", "conv_block_1.0.1.weight", "conv_block_2.2.0.bias", "conv_block_4.1.1.bias",
             "gate.conv.0.bias", "gate.conv.1.weight", "conv_cls.weight", "conv_reg.weight", "conv_reg.bias"]
    params = dict(mref.named_parameters())
    for k in whole:
        g["sd_grad_" + k.replace(".", "_")] = params[k].grad.numpy()
    g["sd_grad_conv_block_3_0_0_weight_head"] = params["conv_block_3.0.0.weight"].grad[:8].numpy()
    g["sd_grad_gate_conv_0_weight_head"] = params["gate.conv.0.weight"].grad[:4].numpy()
    # the same step with the reference's modules in float64 (its loss adapter casts to float32, so the adapter's
    # formulas -- eval_utils.py:51-75 -- are applied to the float64 outputs here): how far the reference's OWN
    # float32 gradients are from the exact ones is the yardstick for the device's
    torch.manual_seed(3)
    m64 = spaam.SpatialDROW(num_scans=5, num_pts=56, alpha=0.5, window_size=11, pedestrian_only=True).double()
    m64.train()
    pc64, pr64, _ = m64(xin.double())
    tcl, trg = torch.from_numpy(tc).long().view(-1), torch.from_numpy(tr).double().view(-1, 2)
    cl64 = m64.cls_loss(torch.sigmoid(pc64.view(-1, 1).squeeze(-1)), tcl.double(), reduction="mean")
    fg = tcl.ne(0)
    rg64 = torch.sqrt(torch.sum(torch.nn.functional.mse_loss(pr64.view(-1, 2)[fg], trg[fg], reduction="none"), dim=1)).mean()
    (cl64 + rg64).backward()
    g["sd64_loss"] = np.array([float((cl64 + rg64).detach()), float(cl64.detach()), float(rg64.detach())])
    p64 = dict(m64.named_parameters())
    g["sd64_gsum"] = np.array([float(p.grad.sum()) for _, p in m64.named_parameters()])
    g["sd64_gabs"] = np.array([float(p.grad.abs().sum()) for _, p in m64.named_parameters()])
    for k in whole:
        g["sd64_grad_" + k.replace(".", "_")] = p64[k].grad.numpy()
    g["sd64_grad_conv_block_3_0_0_weight_head"] = p64["conv_block_3.0.0.weight"].grad[:8].numpy()
    g["sd64_grad_gate_conv_0_weight_head"] = p64["gate.conv.0.weight"].grad[:4].numpy()
    bufs = dict(mref.named_buffers())
    g["sd_run_mean_b1"] = bufs["conv_block_1.0.1.running_mean"].numpy()
    g["sd_run_var_b4"] = bufs["conv_block_4.1.1.running_var"].numpy()
    # ---- N2: one Prototype training step (EPE loss of prototype.py:27-32)
    torch.manual_seed(7)
    pref = proto.Prototype(in_channel=1, max_displacement=5)
    pref.train()
    s1, s2 = torch.randn(3, 450, 1), torch.randn(3, 450, 1)
    tgt = torch.randn(3, 450, 2) * 0.2
    pred = pref(s1, s2)
    ploss, _ = proto.flow_loss(pred, tgt)
    ploss.backward()
    g["pt_s1"], g["pt_s2"], g["pt_tgt"] = s1.numpy(), s2.numpy(), tgt.numpy()
    g["pt_pred"], g["pt_loss"] = pred.detach().numpy(), np.array(float(ploss.detach()))
    g["pt_names"] = np.array([k for k, _ in pref.named_parameters()])
    g["pt_gsum"] = np.array([float(p.grad.double().sum()) for _, p in pref.named_parameters()])
    g["pt_gabs"] = np.array([float(p.grad.double().abs().sum()) for _, p in pref.named_parameters()])
    first = next(iter(pref.named_parameters()))
    g["pt_grad_first"] = first[1].grad.numpy()
    g["pt_first_name"] = np.array(first[0])
    # ---- N2 / configs[3]: one box-head training step (model_fn's loss; dropout off so the step is deterministic),
    #      float32 as the reference runs plus the float64 yardstick                 box_regression.py:20-143
    from src.model.get_model import get_model as ref_get_model
    cfg_b = {"type": "box_reg", "input_dim": 3, "target_dim": 3, "dropout": 0.0}
    torch.manual_seed(67)
    bref = ref_get_model(cfg_b)
    bref.train()
    b64 = ref_get_model(cfg_b).double()
    b64.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in bref.state_dict().items()})
    b64.train()
    bx, bt = torch.randn(48, 64, 3), torch.randn(48, 3)
    bp = bref(bx)
    bl = bref.loss_fn(bp, bt)
    bl.backward()
    bl64 = b64.loss_fn(b64(bx.double()), bt.double())
    bl64.backward()
    used = [(k, p) for k, p in bref.named_parameters() if p.grad is not None]
    g["bh_in"], g["bh_tgt"], g["bh_pred"], g["bh_loss"] = bx.numpy(), bt.numpy(), bp.detach().numpy(), np.array(float(bl.detach()))
    g["bh_names"] = np.array([k for k, _ in used])
    g["bh_gsum"] = np.array([float(p.grad.double().sum()) for _, p in used])
    g["bh_gabs"] = np.array([float(p.grad.double().abs().sum()) for _, p in used])
    p64 = dict(b64.named_parameters())
    g["bh64_loss"] = np.array(float(bl64.detach()))
    g["bh64_gsum"] = np.array([float(p64[k].grad.sum()) for k, _ in used])
    g["bh64_gabs"] = np.array([float(p64[k].grad.abs().sum()) for k, _ in used])
    for k in ("backbone.conv1.0.weight", "backbone.conv3.0.weight", "backbone.conv4.1.weight", "fc3.weight"):
        g["bh_grad_" + k.replace(".", "_")] = dict(used)[k].grad.numpy()
        g["bh64_grad_" + k.replace(".", "_")] = p64[k].grad.numpy()
    g["bh_run_var_c4"] = dict(bref.named_buffers())["backbone.conv4.1.running_var"].numpy()
    np.savez_compressed(os.path.join(OUT, "gradients.npz"), **g)


def gen_person_flow():
    """N5: the per-person tail of depracted_scripts/infer_person_flow.py:134-157, driven through the reference's own
    functions on seeded predictions: u.nms_predicted_center, u.canonical_to_global_flow_torch (float32),
    u._phi_to_rotation_matrix, u.flow_to_hsv, and the script's np.matmul / np.mean lines.  Scores are distinct (the
    reference's argsort is unstable on ties); some flow vectors are exactly zero."""
    import src.utils.utils as u
    from planar_optical_flow_amd import synth
    rng = np.random.default_rng(1701)
    B, N = 4, 450
    phi = u.get_laser_phi()
    scans = np.stack([synth.make_batch(seed=300 + b, B=1, T=1).scans[0, 0] for b in range(B)])
    g = {k: [] for k in ("cls", "reg", "flow", "odom0", "odom1", "inst", "flow_global", "flow_world", "rgb")}
    per_det = {k: [] for k in ("dets_xy", "dets_cls", "dets_xy_world", "det_flow", "det_rgb", "det_count")}
    num = []
    for b in range(B):
        logit = rng.permutation(N).astype(np.float64) / N * 8.0 - 4.0 + rng.uniform(0, 1e-4)
        pred_cls = (1.0 / (1.0 + np.exp(-logit))).reshape(N, 1)                  # distinct sigmoid scores
        pred_reg = rng.normal(0, 0.3, (N, 2))
        flow = rng.normal(0, 0.06, (N, 2)).astype(np.float32)
        flow[rng.random(N) < 0.1] = 0.0
        odom0 = np.array([rng.uniform(40, 80), rng.uniform(80, 120), rng.uniform(-np.pi, np.pi)])
        odom1 = odom0 + np.array([rng.normal(0, 0.05), rng.normal(0, 0.05), rng.normal(0, 0.03)])
        if b == 3:
            odom1[:2] = odom0[:2]                                                # no translation: zero flow stays zero
        pred_flow = u.canonical_to_global_flow_torch(torch.from_numpy(flow), phi).data.cpu().numpy()
        dets_xy, dets_cls, instance_mask = u.nms_predicted_center(scans[b], phi, pred_cls, pred_reg)
        odom_rot = u._phi_to_rotation_matrix(odom1[2])
        dets_xy_world = np.matmul(dets_xy, odom_rot.T) + odom1[:2].reshape(1, 2)
        pred_flow_world = np.matmul(pred_flow, odom_rot.T) + (odom1 - odom0)[:2].reshape(1, 2)
        pred_flow_world_hsv = u.flow_to_hsv(pred_flow_world)
        with np.errstate(all="ignore"), __import__("warnings").catch_warnings():
            __import__("warnings").simplefilter("ignore")
            for j in range(len(dets_xy)):
                instance_ids = instance_mask == j + 1
                per_det["det_flow"].append([np.mean(pred_flow_world[instance_ids, 0]),
                                            np.mean(pred_flow_world[instance_ids, 1])])
                per_det["det_rgb"].append(np.mean(pred_flow_world_hsv[instance_ids], axis=0))
                per_det["det_count"].append(int(instance_ids.sum()))
        per_det["dets_xy"].append(dets_xy), per_det["dets_cls"].append(dets_cls[:, 0])
        per_det["dets_xy_world"].append(dets_xy_world)
        num.append(len(dets_xy))
        for k, v in (("cls", pred_cls), ("reg", pred_reg), ("flow", flow), ("odom0", odom0), ("odom1", odom1),
                     ("inst", instance_mask), ("flow_global", pred_flow), ("flow_world", pred_flow_world),
                     ("rgb", pred_flow_world_hsv)):
            g[k].append(v)
    out = {k: np.stack(v) for k, v in g.items()}
    assert out["flow_global"].dtype == np.float32 and out["flow_world"].dtype == np.float64
    out["scans"], out["num"] = scans, np.array(num, dtype=np.int32)
    for k in ("dets_xy", "dets_cls", "dets_xy_world"):
        out[k] = np.concatenate(per_det[k])
    out["det_flow"], out["det_rgb"] = np.array(per_det["det_flow"]), np.array(per_det["det_rgb"])
    out["det_count"] = np.array(per_det["det_count"], dtype=np.int32)
    np.savez_compressed(os.path.join(OUT, "person_flow.npz"), **out)
    print("person_flow.npz:", {k: v.shape for k, v in out.items()}, "empty detections:",
          int((out["det_count"] == 0).sum()), os.path.getsize(os.path.join(OUT, "person_flow.npz")), "bytes")


def main():
    _install_stubs()
    if "--only" in sys.argv:
        os.makedirs(OUT, exist_ok=True)
        for name in sys.argv[sys.argv.index("--only") + 1:]:
            globals()["gen_" + name]()
        return
    import src.utils.utils as u
    from src.utils.dataset_dr_spaam import DROWDataset2
    from src.depracted.model import prototype as proto
    from src.depracted.model import dr_spaam as spaam
    from src.utils import eval_utils

    from planar_optical_flow_amd import synth

    os.makedirs(OUT, exist_ok=True)
    ds = DROWDataset2.__new__(DROWDataset2)  # only the two stateless mask helpers are used

    # ---------------- A1: angle grids ---------------------------------------
    np.savez_compressed(
        os.path.join(OUT, "phi.npz"),
        phi_450=u.get_laser_phi(),
        phi_3600=u.get_laser_phi(np.radians(0.1), 3600),
        phi_225=u.get_laser_phi(np.radians(1.0), 225),
    )

    # ---------------- A2-A7 on a seeded batch -------------------------------
    B = 6
    sb = synth.make_batch(seed=1, B=B, T=2, mixed_classes=True)
    phi = u.get_laser_phi()
    g = {"seed": 1, "B": B}
    xy, disp, disp_c, ft, ft_c, vel, back = [], [], [], [], [], [], []
    cls_all, reg_all, cls_ped, reg_ped, closest, dyn, valid = [], [], [], [], [], [], []
    for b in range(B):
        cur = sb.scans[b, -1]
        o0, o1 = sb.odom0[b], sb.odom1[b]
        p = np.array(u.rphi_to_xy(cur, phi)).T
        xy.append(p)
        d = u.get_displacement_from_odometry(p, o0, o1)
        disp.append(d)
        dc = u.global_to_canonical_flow(d, phi)
        disp_c.append(dc)
        back.append(u.canonical_to_global_flow(dc, phi))
        ft.append(u.get_flow_target(cur, phi, o0, o1))
        ft_c.append(u.get_flow_target(cur, phi, o0, o1, to_canonical=True))
        vel.append(u.get_velocity_from_odometry(p, o0, o1))
        de = sb.dets[b]
        wc, wa, wp = [list(map(tuple, de[k])) for k in ("wc", "wa", "wp")]
        c, r = u.get_regression_target(cur, phi, wc, wa, wp)
        cls_all.append(c)
        reg_all.append(r)
        c, r = u.get_regression_target(cur, phi, wc, wa, wp, pedestrian_only=True)
        cls_ped.append(c)
        reg_ped.append(r)
        dets = wc + wa + wp
        radii = [0.6] * len(wc) + [0.4] * len(wa) + [0.35] * len(wp)
        closest.append(np.asarray(u.closest_detection(cur, phi, dets, radii), dtype=np.int64))
        dyn.append(ds._get_dynamic_mask(p, wc, wa, wp))
        valid.append(ds._get_valid_point_mask(cur))
    g.update(xy=np.array(xy), disp=np.array(disp), disp_canonical=np.array(disp_c),
             disp_back=np.array(back), flow_target=np.array(ft), flow_target_canonical=np.array(ft_c),
             velocity=np.array(vel), target_cls=np.array(cls_all), target_reg=np.array(reg_all),
             target_cls_ped=np.array(cls_ped), target_reg_ped=np.array(reg_ped),
             closest=np.array(closest), dynamic_mask=np.array(dyn), valid_mask=np.array(valid))
    # odometry stored as float32 on disk in DROW (.odom2 'f4'): second variant
    o0f, o1f = sb.odom0.astype(np.float32), sb.odom1.astype(np.float32)
    g["disp_f32odom"] = np.array([u.get_displacement_from_odometry(np.array(xy[b]), o0f[b], o1f[b])
                                  for b in range(B)])
    # A5 round trip on random regression offsets
    rng = np.random.default_rng(11)
    dx, dy = rng.uniform(-0.5, 0.5, 450), rng.uniform(-0.5, 0.5, 450)
    dr, dp = u.canonical_to_global(sb.scans[0, -1], phi, dx, dy)
    cx, cy = u.global_to_canonical(sb.scans[0, -1], phi, dr, dp)
    g.update(a5_dx=dx, a5_dy=dy, a5_det_r=dr, a5_det_phi=dp, a5_back_x=cx, a5_back_y=cy)
    # A3c
    odt = 0.08
    od = np.array([0.03, -0.01, 0.02])
    g.update(a3c_odom_t=odt, a3c_odom=od)
    # bin/data_prepare.py is a script (runs on import): execute only its
    # get_flow_target definition, taken from the parsed module
    import ast
    src_path = os.path.join(REF, "bin", "data_prepare.py")
    tree = ast.parse(open(src_path).read(), src_path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "get_flow_target"]
    ns = {"np": np, "rphi_to_xy": u.rphi_to_xy}
    exec(compile(ast.Module(body=fn, type_ignores=[]), src_path, "exec"), ns)
    g["a3c_flow"] = ns["get_flow_target"](sb.scans[0, -1], phi, odt, od)
    np.savez_compressed(os.path.join(OUT, "scan_geometry.npz"), **g)

    # ---------------- A8: cutouts -------------------------------------------
    cases = {
        # config/config_test.yaml:19-26 (T=10 + cur)
        "config_test": dict(T=11, N=450, inc=0.5, kw=dict(fixed=False, centered=True, window_width=1.0,
                            window_depth=0.5, num_cutout_pts=56, padding_val=29.99, area_mode=True)),
        # config/dr_spaam.yaml:20-27 (T=5 + cur)
        "dr_spaam": dict(T=6, N=450, inc=0.5, kw=dict(fixed=True, centered=True, window_width=1.0,
                         window_depth=0.5, num_cutout_pts=56, padding_val=29.99, area_mode=True)),
        # function defaults (utils.py:259-270), no area mode, not centred
        "defaults": dict(T=3, N=450, inc=0.5, kw=dict(centered=False)),
        # stride 2, odd sizes, non-power-of-two depth
        "stride2": dict(T=2, N=450, inc=0.5, kw=dict(stride=2, fixed=True, window_width=1.3,
                        window_depth=0.7, num_cutout_pts=32, padding_val=29.99, area_mode=True)),
        # BASELINE config 5 geometry: 3600 pts at 0.1 deg
        "dense3600": dict(T=2, N=3600, inc=0.1, kw=dict(fixed=True, centered=True, window_width=1.0,
                          window_depth=0.5, num_cutout_pts=56, padding_val=29.99, area_mode=True)),
    }
    gc = {}
    for i, (name, c) in enumerate(cases.items()):
        nb = 1 if name in ("config_test", "dense3600") else 2
        sbc = synth.make_batch(seed=100 + i, B=nb, T=c["T"], N=c["N"], angle_inc=np.radians(c["inc"]))
        ph = u.get_laser_phi(np.radians(c["inc"]), c["N"])
        gc[name + "_scans"] = sbc.scans
        gc[name + "_out"] = np.array([u.scans_to_cutout(sbc.scans[b], ph, **c["kw"]) for b in range(nb)])
    # a near-field sample that drives s_area high (ranges down to the 1 cm clamp)
    rng = np.random.default_rng(7)
    near = rng.uniform(0.005, 0.6, (1, 3, 450)).astype(np.float32)
    gc["near_scans"] = near
    gc["near_out"] = np.array([u.scans_to_cutout(near[0], phi, **cases["dr_spaam"]["kw"])])
    np.savez_compressed(os.path.join(OUT, "cutout.npz"), **gc)

    # ---------------- A11: NMS ----------------------------------------------
    rng = np.random.default_rng(21)
    gn = {}
    for k in range(3):
        sbn = synth.make_batch(seed=200 + k, B=1, T=1)
        scan = sbn.scans[0, 0]
        pc = rng.permutation(450).astype(np.float64).reshape(450, 1) / 450.0 + rng.uniform(0, 1e-4)
        pr = rng.normal(0, 0.3, (450, 2))
        xy_, cl_, inst_ = u.nms_predicted_center(scan, phi, pc, pr, min_dist=0.5)
        gn.update({f"scan{k}": scan, f"cls{k}": pc, f"reg{k}": pr, f"xy{k}": xy_, f"keepcls{k}": cl_,
                   f"inst{k}": inst_})
    np.savez_compressed(os.path.join(OUT, "nms.npz"), **gn)

    # ---------------- A12: losses -------------------------------------------
    rng = np.random.default_rng(31)
    pred = rng.normal(0, 0.1, (5, 450, 2)).astype(np.float32)
    tgt = rng.normal(0, 0.1, (5, 450, 2)).astype(np.float32)
    msk = (rng.random((5, 450)) < 0.8).astype(np.float32)
    tp, tt, tm = map(torch.from_numpy, (pred, tgt, msk))
    l_proto, err_b = proto.flow_loss(tp, tt)
    l_mask = spaam.flow_loss(tp, tt, tm)
    l_nomask = spaam.flow_loss(tp, tt)
    epe_b, aae_b = eval_utils.loss_fn_eval(tp, tt)
    np.savez_compressed(os.path.join(OUT, "losses.npz"), pred=pred, target=tgt, mask=msk,
                        proto_loss=l_proto.numpy(), proto_err=err_b.numpy(), masked=l_mask.numpy(),
                        unmasked=l_nomask.numpy(), epe=epe_b.numpy(), aae=aae_b.numpy())

    # ---------------- A9: banded patch correlation --------------------------
    torch.manual_seed(41)
    f1, f2 = torch.randn(2, 256, 57), torch.randn(2, 256, 57)
    fused = proto.Prototype._fusion(None, f1, f2)
    f1s, f2s = torch.randn(3, 16, 23), torch.randn(3, 16, 23)
    fused_s = proto.Prototype._fusion(None, f1s, f2s, kernel_size=3, max_displacement=3)
    np.savez_compressed(os.path.join(OUT, "band_corr.npz"), f1=f1.numpy(), f2=f2.numpy(), out=fused.numpy(),
                        f1s=f1s.numpy(), f2s=f2s.numpy(), outs=fused_s.numpy())

    # ---------------- A10: spatial attention --------------------------------
    torch.manual_seed(51)
    n_cut, n_ch, n_pts = 40, 32, 14
    att = spaam._SpatialAttention(n_pts=n_pts, n_channel=n_ch, alpha=0.5, window_size=11)
    att.eval()
    with torch.no_grad():
        att.conv[1].running_mean.normal_(0, 0.1)
        att.conv[1].running_var.uniform_(0.5, 1.5)
        x = torch.randn(2, n_cut, n_ch, n_pts)
        t = torch.randn(2, n_cut, n_ch, n_pts)
        out, band = att(x, t)
        emb_x = att.conv(x.view(2 * n_cut, n_ch, n_pts)).view(2, n_cut, 128)
        emb_t = att.conv(t.view(2 * n_cut, n_ch, n_pts)).view(2, n_cut, 128)
    sd = {"sd_" + k.replace(".", "_"): v.numpy() for k, v in att.state_dict().items()}
    np.savez_compressed(os.path.join(OUT, "spatial_attn.npz"), x=x.numpy(), tmpl=t.numpy(), out=out.numpy(),
                        band=band.numpy(), emb_x=emb_x.numpy(), emb_t=emb_t.numpy(), **sd)
    # a window of 7 with alpha 0.3 on odd sizes
    torch.manual_seed(52)
    att2 = spaam._SpatialAttention(n_pts=5, n_channel=8, alpha=0.3, window_size=7)
    att2.eval()
    with torch.no_grad():
        x2, t2 = torch.randn(1, 19, 8, 5), torch.randn(1, 19, 8, 5)
        out2, band2 = att2(x2, t2)
        e2x = att2.conv(x2.view(19, 8, 5)).view(1, 19, 128)
        e2t = att2.conv(t2.view(19, 8, 5)).view(1, 19, 128)
    np.savez_compressed(os.path.join(OUT, "spatial_attn_w7.npz"), x=x2.numpy(), tmpl=t2.numpy(),
                        out=out2.numpy(), band=band2.numpy(), emb_x=e2x.numpy(), emb_t=e2t.numpy())

    # ---------------- A14: box head forward (weights rebuilt from the seed) ---
    from src.model.get_model import get_model as ref_get_model
    from src.model.box_regression import regression_loss2 as ref_loss2
    gb = {}
    for tag, cfg_m, npts in (("2d", {"type": "box_reg", "input_dim": 3, "target_dim": 3, "dropout": 0.3}, 64),
                             ("3d", {"type": "box_reg", "input_dim": 4, "target_dim": 5, "dropout": 0.3}, 256)):
        torch.manual_seed(61)
        mref = ref_get_model(cfg_m)
        mref.eval()
        xin = torch.randn(4, npts, cfg_m["input_dim"])
        tgt = torch.randn(4, cfg_m["target_dim"])
        with torch.no_grad():
            yout = mref(xin)
            lval = ref_loss2(yout, tgt)
        gb["in_" + tag] = xin.numpy()
        gb["tgt_" + tag] = tgt.numpy()
        gb["out_" + tag] = yout.numpy()
        gb["loss_" + tag] = lval.numpy()
        gb["keys_" + tag] = np.array(list(mref.state_dict().keys()))
        gb["abs_sum_" + tag] = np.array([float(v.abs().sum()) for v in mref.state_dict().values()])
    np.savez_compressed(os.path.join(OUT, "box_head.npz"), **gb)

    # ---------------- N1: the reference's own Dataset.__getitem__ + collate_batch ----------
    # DROWDataset2 is driven with in-memory synthetic sequences (its __init__ only parses
    # files); every sample then goes through the reference's real __getitem__.
    rng = np.random.default_rng(71)
    ds2 = DROWDataset2.__new__(DROWDataset2)
    ds2._num_scans, ds2._use_data_augmentation = 5, False
    ds2._cutout_kwargs = dict(fixed=True, centered=True, window_width=1.0, window_depth=0.5, num_cutout_pts=56,
                              padding_val=29.99, area_mode=True)
    ds2._network_type, ds2._polar_grid_kwargs, ds2._pedestrian_only = "cutout", None, False
    ds2._scan_stride, ds2._pt_stride, ds2.max_scan_dist = 1, 1, 6
    ds2.seq_names, ds2.scans, ds2.scans_ns, ds2.scans_t = [], [], [], []
    ds2.odoms_t, ds2.odoms, ds2.dets_ns, ds2.dets_wc, ds2.dets_wa, ds2.dets_wp = [], [], [], [], [], []
    ds2.idet2iscan, ds2.flat_seq_inds, ds2.flat_det_inds = [], [], []
    gd = {}
    for q, (S, every) in enumerate(((34, 3), (27, 4))):
        sbq = synth.make_batch(seed=300 + q, B=S, T=1)
        sc = sbq.scans[:, 0]
        ns = np.arange(500 * (q + 1), 500 * (q + 1) + S, dtype=np.uint32)
        st = (np.arange(S) * 0.08 + 3.0 + 0.013 * q).astype(np.float32)
        O = 2 * S + 3
        ot = (np.arange(O) * 0.04 + 2.97).astype(np.float32)
        od = np.cumsum(rng.uniform(-0.02, 0.02, (O, 3)), axis=0).astype(np.float32)
        dns = ns[::every]
        wcs, was, wps = [], [], []
        for _ in dns:
            k = rng.integers(0, 4, 3)
            mk = lambda n: [[float(rng.uniform(1, 8)), float(rng.uniform(-1.6, 1.6))] for _ in range(n)]
            wcs.append(mk(k[0])); was.append(mk(k[1])); wps.append(mk(k[2]))
        ds2.seq_names.append("seq%d" % q); ds2.scans.append(sc); ds2.scans_ns.append(ns); ds2.scans_t.append(st)
        ds2.odoms_t.append(ot); ds2.odoms.append(od); ds2.dets_ns.append(dns)
        ds2.dets_wc.append(wcs); ds2.dets_wa.append(was); ds2.dets_wp.append(wps)
        m = {i: int(np.where(ns == d)[0][0]) for i, d in enumerate(dns)}
        ds2.idet2iscan.append(m)
        ds2.flat_seq_inds += [q] * len(m)
        ds2.flat_det_inds += list(range(len(m)))
        gd.update({"scans%d" % q: sc, "scans_ns%d" % q: ns, "scans_t%d" % q: st, "odoms_t%d" % q: ot,
                   "odoms%d" % q: od, "dets_ns%d" % q: dns})
        for nm, lst in (("wc", wcs), ("wa", was), ("wp", wps)):
            gd["%s_cnt%d" % (nm, q)] = np.array([len(x) for x in lst], dtype=np.int32)
            gd["%s_val%d" % (nm, q)] = np.array([v for x in lst for v in x], dtype=np.float64).reshape(-1, 2)
    items = [ds2[i] for i in range(len(ds2))]
    coll = ds2.collate_batch(items)
    gd["n_items"] = len(items)
    for k in ("scans", "target_cls", "target_reg", "target_flow", "exclude_mask"):
        gd["out_" + k] = coll[k]
    gd["out_odom1"] = np.array(coll["odom1"])
    gd["out_odom1_t"] = np.array(coll["odom1_t"])
    gd["out_scans_ns"] = np.array(coll["scans_ns"])
    gd["out_dets_ns"] = np.array(coll["dets_ns"])
    gd["out_input_first3"] = coll["input"][:3]
    np.savez_compressed(os.path.join(OUT, "dataset_items.npz"), **gd)

    # ---------------- N1: the reference's file loaders and its __init__ from files ----------
    # Synthetic DROW-format text files (written to a temp dir; their bytes are stored in the
    # fixture so the test can re-create them), parsed by the reference's own loaders, then the
    # reference's real DROWDataset2(data_path, split) -> __getitem__ -> collate_batch.
    import tempfile, json as _json
    rng = np.random.default_rng(72)
    tmp = tempfile.mkdtemp(prefix="pof_drow_")
    os.makedirs(os.path.join(tmp, "train"))
    gf = {}
    names = ["run_a", "run_b", "run_static"]
    for q, nm in enumerate(names):
        S = (31, 26, 12)[q]
        sbq = synth.make_batch(seed=400 + q, B=S, T=1)
        sc = sbq.scans[:, 0]
        ns = np.arange(100 * (q + 1), 100 * (q + 1) + S)
        st = np.arange(S) * 0.08 + 1.5 + 0.01 * q
        od = np.cumsum(rng.uniform(-0.02, 0.02, (S, 3)), axis=0)
        if nm == "run_static":
            od[:] = od[0]                      # dropped by the static-scene filter
        else:
            od[7] = od[6]                      # one repeated odometry row inside a moving sequence
        base = os.path.join(tmp, "train", nm)
        with open(base + ".csv", "w") as f:
            for i in range(S):
                f.write("%d,%.6f,%s\n" % (ns[i], st[i], ",".join("%.3f" % v for v in sc[i])))
        with open(base + ".odom2", "w") as f:
            for i in range(S):
                f.write("%d,%.6f,%.6f,%.6f,%.6f\n" % (ns[i], st[i] - 0.004, od[i, 0], od[i, 1], od[i, 2]))
        dns = ns[2::3]
        for ext in ("wc", "wa", "wp"):
            with open(base + "." + ext, "w") as f:
                for d in dns:
                    k = int(rng.integers(0, 3))
                    dets = [[round(float(rng.uniform(1, 8)), 3), round(float(rng.uniform(-1.6, 1.6)), 4)] for _ in range(k)]
                    f.write("%d,%s\n" % (d, _json.dumps(dets)))
        for ext in ("csv", "odom2", "wc", "wa", "wp"):
            gf["file_%s_%s" % (nm, ext)] = np.frombuffer(open(base + "." + ext, "rb").read(), dtype=np.uint8)
        lo = DROWDataset2.__new__(DROWDataset2)
        a, b, c = lo._load_scan_file(base)
        gf["scan_ns_" + nm], gf["scan_t_" + nm], gf["scan_" + nm] = a, b, c
        a, b, c = lo._load_odom(base)
        gf["odom_ns_" + nm], gf["odom_t_" + nm], gf["odom_" + nm] = a, b, c
        a, wcs, was, wps = lo._load_det_file(base)
        gf["det_ns_" + nm] = a
        for tag, lst in (("wc", wcs), ("wa", was), ("wp", wps)):
            gf["det_%s_cnt_%s" % (tag, nm)] = np.array([len(x) for x in lst], dtype=np.int32)
            gf["det_%s_val_%s" % (tag, nm)] = np.array([v for x in lst for v in x], dtype=np.float64).reshape(-1, 2)
    ckw = dict(fixed=True, centered=True, window_width=1.0, window_depth=0.5, num_cutout_pts=56,
               padding_val=29.99, area_mode=True)
    ds3 = DROWDataset2(tmp, split="train", num_scans=5, network_type="cutout", cutout_kwargs=ckw)
    gf["ds_seq_names"] = np.array([os.path.basename(n) for n in ds3.seq_names])
    gf["ds_flat_seq"] = np.array(ds3.flat_seq_inds, dtype=np.int32)
    gf["ds_flat_scan"] = np.array([ds3.idet2iscan[s][d] for s, d in zip(ds3.flat_seq_inds, ds3.flat_det_inds)],
                                  dtype=np.int32)
    coll3 = ds3.collate_batch([ds3[i] for i in range(len(ds3))])
    for k in ("scans", "target_cls", "target_reg", "target_flow", "exclude_mask"):
        gf["out_" + k] = coll3[k]
    gf["out_odom1"] = np.array(coll3["odom1"])
    gf["out_input_first2"] = coll3["input"][:2]
    np.savez_compressed(os.path.join(OUT, "dataset_files.npz"), **gf)
    import shutil
    shutil.rmtree(tmp)

    # ---------------- N3, file side: the reference's JRDBHandle on a synthetic JRDB tree ---------
    # tests/jrdb_tree.py writes the tree from a seed (ascii and binary .pcd; the LZF encoding needs
    # python-lzf, which this image lacks, and is covered by round-trip tests instead); the reference's
    # handle indexes and reads it.  3-D mode: every labelled frame.  2-D mode: only the frame whose
    # annotation list is empty -- the reference's 2-D branch raises on the first annotation
    # (jrdb_handle.py:250-252 calls list.append with five arguments), so `points` is what it can give.
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import jrdb_tree
    import src.data_handle.jrdb_handle as ref_jh
    tmp = tempfile.mkdtemp(prefix="pof_jrdb_")
    val_names = list(ref_jh._JRDB_VAL_SEQUENCES)
    labelled = jrdb_tree.make_tree(tmp, val_names, seed=11)
    gj = {"val_sequences": np.array(val_names), "train_sequences": np.array(ref_jh._JRDB_TRAIN_SEQUENCES),
          "labelled_seq": np.array([a for a, _, _ in labelled]), "labelled_file": np.array([b for _, b, _ in labelled])}
    h3 = ref_jh.JRDBHandle("val", {"data_dir": tmp, "radius_segment": 0.7, "perturb": 0.1, "is_3d": True})
    gj["len"] = np.array(len(h3))
    for i in range(len(h3)):
        np.random.seed(1000 + i)
        fr = h3[i]
        gj["f%d_points" % i] = fr["points"]
        gj["f%d_boxes" % i] = np.asarray(fr["boxes"], dtype=np.float64)
        gj["f%d_centers" % i] = np.asarray(fr["dets_center"], dtype=np.float64)
        gj["f%d_seg_len" % i] = np.array([len(sg) for sg in fr["segments"]], dtype=np.int32)
        gj["f%d_seg_pts" % i] = np.concatenate(fr["segments"]) if len(fr["segments"]) else np.zeros((0, 3), np.float32)
        gj["f%d_url" % i] = np.array(fr["pointclouds"]["upper_velodyne"]["url"])
    h2 = ref_jh.JRDBHandle("test", {"data_dir": tmp, "radius_segment": 0.7, "perturb": 0.1, "is_3d": False})
    empty = [i for i, (_, _, n) in enumerate(labelled) if n == 0]
    gj["empty_index"] = np.array(empty)
    for i in empty:
        gj["laser%d_points" % i] = h2[i]["points"]
    np.savez_compressed(os.path.join(OUT, "jrdb_files.npz"), **gj)
    shutil.rmtree(tmp)

    # ---------------- N4 + A13: the legacy boosted-stump baseline ---------------------------------
    # src/depracted/model/adaboost_person_det.py is a script: it parses --cfg at import and imports
    # src.data_handle.depracted.drow_handle, a module the reference repository does not contain.  Both
    # are satisfied harness-side (an argv with a throw-away yaml, an empty module with a DROWHandle
    # name) so that its classes can be driven directly; none of them touches the placeholder.
    for modname in ("src.data_handle.depracted", "src.data_handle.depracted.drow_handle"):
        sys.modules[modname] = types.ModuleType(modname)
    sys.modules["src.data_handle.depracted.drow_handle"].DROWHandle = object
    tmp = tempfile.mkdtemp(prefix="pof_ada_")
    with open(os.path.join(tmp, "ada.yaml"), "w") as f:
        f.write("tag: ''\n")
    argv, sys.argv = sys.argv, ["adaboost_person_det", "--cfg", os.path.join(tmp, "ada.yaml")]
    import src.depracted.model.adaboost_person_det as ada
    sys.argv = argv
    shutil.rmtree(tmp)
    ga = {}
    det = ada.BoostedFeatureDetector()
    rng = np.random.default_rng(2024)
    # (a) simple_classifier on tie-free feature tables, one of them resampled with replacement
    shapes = [(40, 3), (200, 14), (333, 6), (64, 1), (200, 9), (120, 5)]
    ga["sc_cases"] = np.array(len(shapes))
    for q, (n, D) in enumerate(shapes):
        X = rng.normal(size=(n, D)) * rng.uniform(0.5, 20, D)
        Y = np.where(X[:, q % D] * 0.7 + rng.normal(size=n) * X[:, q % D].std() * 0.6 > 0.1, 1.0, -1.0)
        if q == 4:                                  # a boosting round: 200 draws out of 90 rows
            pick = rng.integers(0, 90, n)
            X, Y = X[pick], Y[pick]
            ga["sc%d_pick" % q] = pick
        if q == 5:                                  # inverted relation: the 1 - error branch wins
            Y = -Y
        jj, th = det.simple_classifier(X, Y.reshape(-1, 1))
        ga["sc%d_X" % q], ga["sc%d_Y" % q] = X, Y
        ga["sc%d_out" % q] = np.array([jj, th], dtype=np.float64)
    # (b) adaboost + eval, seeded global state; the second table separates early (error < 0.1 -> alpha = 1, stop)
    for q, (N, D, K, ns, noise) in enumerate([(600, 8, 12, 150, 0.8), (400, 5, 6, 100, 0.02)]):
        X = rng.normal(size=(N, D))
        Y = np.where(X[:, 2] + 0.5 * X[:, 0] * (q == 0) + noise * rng.normal(size=N) > 0.0, 1.0, -1.0)
        np.random.seed(50 + q)
        alphaK, para = det.adaboost(X, Y.reshape(-1, 1), K, ns)
        labels, result = det.eval(X, alphaK, para)
        ga["ab%d_X" % q], ga["ab%d_Y" % q] = X, Y
        ga["ab%d_cfg" % q] = np.array([K, ns, 50 + q])
        ga["ab%d_alpha" % q], ga["ab%d_para" % q] = alphaK, para
        ga["ab%d_labels" % q], ga["ab%d_result" % q] = labels, result
    # (c) nms_predicted_center with distinct predictions
    segs = [[rng.normal(size=(int(rng.integers(3, 9)), 2)) * 0.1 + rng.uniform(-3, 3, 2), 1.0] for _ in range(25)]
    preds = rng.permutation(25).astype(np.float64) - 12.5
    scores = rng.uniform(-0.5, 2.0, 25)
    sg, pr, sc = ada.nms_predicted_center(segs, preds.copy(), scores.copy(), min_dist=1.0)
    ga["nms_seg_len"] = np.array([len(x[0]) for x in segs])
    ga["nms_seg_pts"] = np.concatenate([x[0] for x in segs])
    ga["nms_preds"], ga["nms_scores"] = preds, scores
    ga["nms_out_first_pt"] = np.array([x[0] for x in sg])
    ga["nms_out_preds"], ga["nms_out_scores"] = pr, sc
    # (d) A13: scan_to_segments + compute_feature of the reference's Dataset on seeded scans
    phi = u.get_laser_phi()
    scans_a = 6.0 + 0.4 * np.sin(np.arange(450) / 40.0)[None] + 0.01 * rng.normal(size=(3, 450))
    for b in range(3):                              # legs / boxes in front of a wall: >= 4 segments of > 2 points
        at = 10
        while at < 420:
            span = int(rng.integers(3, 26))
            scans_a[b, at:at + span] = rng.uniform(1.5, 4.0) + 0.05 * np.cos(np.linspace(-1.5, 1.5, span)) \
                + 0.004 * rng.normal(size=span)
            at += span + int(rng.integers(1, 40))
    dsa = ada.Dataset.__new__(ada.Dataset)
    dsa.scans_data = []
    for b in range(3):
        scan = scans_a[b]
        segs_b = np.split(np.array(u.rphi_to_xy(scan, phi)).T,
                          np.clip(np.where(np.abs(scan[1:] - scan[:-1]) >= 0.5)[0] + 1, 0, len(scan) - 1))
        big = [sgm for sgm in segs_b if len(sgm) > 2]
        wps = [big[i].mean(axis=0) + 0.05 for i in range(0, len(big), 3)]       # annotations near every third segment
        segments, labels, cut_ids = dsa.scan_to_segments(scan, phi, wps)
        dsa.scans_data.append([[[sgm, lb] for sgm, lb in zip(segments, labels) if len(sgm) > 2], cut_ids, scan, 0.1 * b])
        ga["ft%d_scan" % b], ga["ft%d_wps" % b] = scan, np.array(wps)
        ga["ft%d_cut_ids" % b], ga["ft%d_labels_all" % b] = cut_ids, labels
    for b in range(3):
        ga["ft%d_features" % b] = np.array(dsa.compute_feature(dsa.scans_data[b], b), dtype=np.float64).reshape(-1, 15)
    np.savez_compressed(os.path.join(OUT, "adaboost.npz"), **ga)

    # ---------------- flow_to_hsv (colour coding of flow vectors, used by the evaluation loops) -------
    rh = np.random.default_rng(606)
    fl = np.concatenate([rh.normal(size=(300, 2)) * 0.05, rh.normal(size=(100, 2)), np.zeros((3, 2)),
                         np.array([[0.1, 0.0], [0.0, 0.1], [-0.1, 0.0], [0.0, -0.1], [-1e-9, -0.0]])])
    np.savez_compressed(os.path.join(OUT, "flow_hsv.npz"), flow=fl, rgb=u.flow_to_hsv(fl))

    # ---------------- N4: scans_to_polar_grid -------------------------------------------------
    gp = {}
    sbp = synth.make_batch(seed=81, B=2, T=5)
    cases = [("default", {}), ("raw", dict(normalize=False)), ("noclip", dict(tsdf_clip=0.0)),
             ("fine", dict(min_range=0.5, max_range=25.0, range_bin_size=0.25, tsdf_clip=2.0))]
    for b in range(2):
        gp["scans%d" % b] = sbp.scans[b]
        for tag, kwp in cases:
            gp["out%d_%s" % (b, tag)] = u.scans_to_polar_grid(sbp.scans[b], **kwp)
    np.savez_compressed(os.path.join(OUT, "polar_grid.npz"), **gp)

    # ---------------- N2: DROW / SpatialDROW forward (weights rebuilt from the seed) ------------
    gm = {}
    torch.manual_seed(3)
    mref = spaam.SpatialDROW(num_scans=5, num_pts=56, alpha=0.5, window_size=11, pedestrian_only=True)
    gm["keys"] = np.array(list(mref.state_dict().keys()))
    gm["abs_sum"] = np.array([float(v.double().abs().sum()) for v in mref.state_dict().values()])
    xin = torch.randn(2, 30, 5, 56) * 0.5
    gm["x"] = xin.numpy()
    mref.eval()
    with torch.no_grad():
        pc, pr, ff = mref(xin)
        gm["eval_cls"], gm["eval_reg"], gm["eval_feat"] = pc.numpy(), pr.numpy(), ff.numpy()
        # streaming inference: two consecutive scans through the running template
        c0, r0, tmpl0, f0 = mref(xin[:, :, 3:4], testing=True)
        c1, r1, tmpl1, f1 = mref(xin[:, :, 4:5], testing=True, fea_template=tmpl0)
        gm["stream_cls"], gm["stream_reg"], gm["stream_feat"] = c1.numpy(), r1.numpy(), f1.numpy()
    mref.train()
    pc, pr, ff = mref(xin)                       # BatchNorm with batch statistics
    gm["train_cls"], gm["train_reg"], gm["train_feat"] = pc.detach().numpy(), pr.detach().numpy(), ff.detach().numpy()
    torch.manual_seed(4)
    dref = spaam.DROW(num_scans=5, num_pts=48)
    dref.eval()
    xd = torch.randn(2, 25, 5, 48) * 0.5
    with torch.no_grad():
        dc, dr_ = dref(xd)
    gm["drow_x"], gm["drow_cls"], gm["drow_reg"] = xd.numpy(), dc.numpy(), dr_.numpy()
    # the detector's loss adapter on both heads (one-logit sigmoid / BCE, four-class cross entropy)
    torch.manual_seed(3)                          # a fresh copy: the train-mode forward above moved the BatchNorm statistics
    mref = spaam.SpatialDROW(num_scans=5, num_pts=56, alpha=0.5, window_size=11, pedestrian_only=True)
    mref.eval()
    rs = np.random.default_rng(17)
    tc1 = (rs.uniform(size=(2, 30)) < 0.3).astype(np.int64)
    tr1 = rs.normal(size=(2, 30, 2)).astype(np.float32)
    with torch.no_grad():
        l1, tb1, _ = eval_utils.model_fn_obj_det(mref, {"input": xin.numpy(), "target_flow_cls": tc1, "target_flow_reg": tr1})
    gm["objdet1_cls"], gm["objdet1_reg"] = tc1, tr1
    gm["objdet1_out"] = np.array([float(l1), tb1["cls_loss"], tb1["fg_ratio"], tb1["reg_loss"]])
    tc4 = rs.integers(0, 4, (2, 25)).astype(np.int64)
    tr4 = rs.normal(size=(2, 25, 2)).astype(np.float32)
    with torch.no_grad():
        l4, tb4, _ = eval_utils.model_fn_obj_det(dref, {"input": xd.numpy(), "target_flow_cls": tc4, "target_flow_reg": tr4})
        l0, tb0, _ = eval_utils.model_fn_obj_det(dref, {"input": xd.numpy(), "target_flow_cls": tc4 * 0, "target_flow_reg": tr4})
    gm["objdet4_cls"], gm["objdet4_reg"] = tc4, tr4
    gm["objdet4_out"] = np.array([float(l4), tb4["cls_loss"], tb4["fg_ratio"], tb4["reg_loss"]])
    gm["objdet0_out"] = np.array([float(l0), tb0["cls_loss"], tb0["fg_ratio"]])        # no foreground: no reg term
    np.savez_compressed(os.path.join(OUT, "dr_spaam_model.npz"), **gm)

    # ---------------- N2: Prototype flow network (weights rebuilt from the seed) ----------------
    from src.depracted.model import prototype as proto
    gq = {}
    torch.manual_seed(7)
    pref = proto.Prototype(in_channel=1, max_displacement=5)
    gq["keys"] = np.array(list(pref.state_dict().keys()))
    gq["abs_sum"] = np.array([float(v.double().abs().sum()) for v in pref.state_dict().values()])
    s1, s2 = torch.randn(3, 450, 1), torch.randn(3, 450, 1)
    pref.eval()
    with torch.no_grad():
        gq["eval_out"] = pref(s1, s2).numpy()
    pref.train()
    gq["train_out"] = pref(s1, s2).detach().numpy()
    gq["s1"], gq["s2"] = s1.numpy(), s2.numpy()
    np.savez_compressed(os.path.join(OUT, "prototype_model.npz"), **gq)

    gen_rotate_iou()
    gen_cutout_dense()
    gen_cutout_indices()
    gen_gradients()
    gen_person_flow()

    tot = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    print("wrote", sorted(os.listdir(OUT)), "total bytes", tot)


if __name__ == "__main__":
    main()
