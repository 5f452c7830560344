"""Kernel forms that the host launchers choose from the SIZE of a launch.  The conv trunk launcher picks 32, 64 or 128
output channels per workgroup (and a split-K form for small launches) from how many workgroups the batch makes; the
spatial attention walks pick their segment length from the batch.  The rest of the suite runs small batches, so only
the small-launch forms; here every case first asserts the form the host-only plan query (ops.conv1d_plan,
ops.spatial_attention_plan) reports for its size, then checks the numbers against float64 torch: exactly on integer
data, at the existing float bar on random data, and bit for bit against small launches of the same sequences / rows
where the summation order does not depend on the form.  The training tail (BatchNorm statistics, weight gradient)
runs at the reference's training batch.
"""
import pytest
import torch
import torch.nn.functional as F

from cases import (ATTENTION_CASES, ATTENTION_E, ATTENTION_F, ATTENTION_W, BN_TAIL_CASES, CONV_FAMILIES,
                   CONV_FORM_CASES, CONV_WIDE_CASE, WGRAD_CASES, conv_case_batch)
from test_hip_parity import _torch_attention

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from planar_optical_flow_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _ops


@pytest.fixture(autouse=True)
def _release_memory():
    yield
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- conv trunk forms
def _conv(ops, family, x, w, scale, shift, pool, slope, table=None, slope1=0.0):
    """The layer through the entry point of its family; w [Co, Ci, k] as torch stores it."""
    kernel, stride = CONV_FAMILIES[family]
    wt = w.permute(2, 1, 0).contiguous()
    if family == "fused":
        return ops.conv3_first_two(x, table, wt, scale, shift, slope1=slope1, pool=pool, negative_slope=slope)
    if family == "k3s1":
        return ops.conv3_bn_lrelu(x, wt, scale, shift, pool=pool, negative_slope=slope)
    return ops.conv1d_bn_lrelu(x, wt, scale, shift, stride=stride, pool=pool, negative_slope=slope)


def _conv_reference(family, x, w, scale, shift, pool, slope, table=None, slope1=0.0):
    """float64 torch: [first unit ->] Conv1d -> scale / shift -> LeakyReLU [-> max_pool1d 2], in sequence chunks of
    about 256 MB; rounded to float32 once at the end."""
    kernel, stride = CONV_FAMILIES[family]
    S, L = x.shape[0], x.shape[-1]
    per = max(1, (1 << 25) // (max(w.shape[0], w.shape[1]) * L))
    w64, sc64, sh64 = w.double(), scale.double()[:, None], shift.double()[:, None]
    out = []
    for s0 in range(0, S, per):
        xs = x[s0:s0 + per].double()
        if table is not None:                 # x [S, L]: the single-channel first unit, {a0, a1, a2, b} per channel
            t = table.double()
            xs = F.leaky_relu(F.conv1d(xs[:, None, :], t[:, None, :3], t[:, 3], padding=1), slope1)
        y = F.leaky_relu(F.conv1d(xs, w64, None, stride=stride, padding=kernel // 2) * sc64 + sh64, slope)
        out.append((F.max_pool1d(y, 2) if pool else y).float())
    return torch.cat(out)


def _conv_id(case):
    family, Ci, Co, L, pool, cpw, split, quantised = case
    return "%s-%dx%d-L%d%s-%s%d%s" % (family, Ci, Co, L, "-pool" if pool else "", "splitk" if split else "ct", cpw,
                                      "q" if quantised else "")


@pytest.mark.parametrize("case", CONV_FORM_CASES, ids=_conv_id)
def test_conv_form_vs_float64(ops, case):
    """Each form of the trunk conv at the smallest batch that runs it: exact on integer data, 1e-4 on random data, and
    three 8-sequence slices bit-identical to separate small launches (which run narrower channel groups with the same
    summation order) -- to the float bar where either launch is split-K, which sums K in another order."""
    family, Ci, Co, L, pool, cpw, split, quantised = case
    kernel, stride = CONV_FAMILIES[family]
    fused = family == "fused"
    S = conv_case_batch(ops.conv1d_plan, case)
    plan = ops.conv1d_plan(S, Ci, Co, L, kernel, stride, pool, fused)
    assert plan == dict(split_k=split, channels_per_workgroup=cpw, launches=1, wide_offsets=0), (S, plan)
    gen = torch.Generator(device=DEV).manual_seed(S * 7 + Ci * 131 + Co + L)
    xshape = (S, L) if fused else (S, Ci, L)

    # integer data, power-of-two scale and slopes: every float32 operation is exact
    x = torch.randint(-3, 4, xshape, generator=gen, device=DEV).float()
    w = torch.randint(-2, 3, (Co, Ci, kernel), generator=gen, device=DEV).float()
    scale = torch.full((Co,), 0.5, device=DEV)
    shift = torch.randint(-4, 5, (Co,), generator=gen, device=DEV).float()
    table = torch.randint(-2, 3, (Ci, 4), generator=gen, device=DEV).float() if fused else None
    got = _conv(ops, family, x, w, scale, shift, pool, 0.125, table, 0.5)
    want = _conv_reference(family, x, w, scale, shift, pool, 0.125, table, 0.5)
    assert got.shape == want.shape
    assert torch.equal(got, want), (S, (got - want).abs().max().item())

    x = torch.randn(xshape, generator=gen, device=DEV)
    w = torch.randn((Co, Ci, kernel), generator=gen, device=DEV) / (kernel * Ci) ** 0.5
    scale = torch.rand((Co,), generator=gen, device=DEV) + 0.5
    shift = torch.randn((Co,), generator=gen, device=DEV)
    if fused:
        table = torch.cat((torch.randn((Ci, 3), generator=gen, device=DEV) * 0.5,
                           torch.randn((Ci, 1), generator=gen, device=DEV) * 0.2), dim=1).contiguous()
    got = _conv(ops, family, x, w, scale, shift, pool, 0.1, table, 0.1)
    want = _conv_reference(family, x, w, scale, shift, pool, 0.1, table, 0.1)
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-5)
    small = ops.conv1d_plan(8, Ci, Co, L, kernel, stride, pool, fused)
    for lo in (0, S // 2 - 4, S - 8):
        sub = _conv(ops, family, x[lo:lo + 8].contiguous(), w, scale, shift, pool, 0.1, table, 0.1)
        if split or small["split_k"]:
            torch.testing.assert_close(sub, got[lo:lo + 8], rtol=1e-4, atol=1e-5)
        else:
            assert torch.equal(sub, got[lo:lo + 8]), (lo, small, (sub - got[lo:lo + 8]).abs().max().item())


def test_conv_wide_output_offsets(ops):
    """One launch that writes more than 2^30 output elements takes 64-bit output offsets in the epilogue: sequences at
    the start, either side of element 2^30 and at the end, exactly against float64."""
    family, Ci, Co, L, pool, S = CONV_WIDE_CASE
    plan = ops.conv1d_plan(S, Ci, Co, L, 3, 1, pool)
    assert plan == dict(split_k=False, channels_per_workgroup=128, launches=1, wide_offsets=1), plan
    gen = torch.Generator(device=DEV).manual_seed(78)
    x = torch.randint(-2, 3, (S, Ci, L), generator=gen, device=DEV, dtype=torch.int8).float()
    w = torch.randint(-2, 3, (Co, Ci, 3), generator=gen, device=DEV, dtype=torch.int8).float()
    scale = torch.full((Co,), 0.25, device=DEV)
    shift = torch.randint(-2, 3, (Co,), generator=gen, device=DEV).float()
    got = _conv(ops, family, x, w, scale, shift, pool, 0.125)
    Lout = L // 2 if pool else L
    edge = (1 << 30) // (Co * Lout)                      # the sequence that holds output element 2^30
    for lo, hi in ((0, 40), (edge - 40, edge + 40), (S - 40, S)):
        want = _conv_reference(family, x[lo:hi], w, scale, shift, pool, 0.125)
        assert torch.equal(got[lo:hi], want), (lo, hi, (got[lo:hi] - want).abs().max().item())


def test_dr_spaam_forward_at_readme_batch(ops):
    """SpatialDROW at the README's 32 windows x 450 cutouts x 5 scans x 56 points: the HIP trunk
    (fuse_for_inference) against the module path, at the bar test_spatial_drow_forward_equals_reference uses."""
    from planar_optical_flow_amd.src.depracted.model.dr_spaam import SpatialDROW
    B, N, T, P = 32, 450, 5, 56
    S12, S34 = B * N * T, B * N                      # blocks 1-2 take every scan, blocks 3-4 the fused template
    form = lambda *a, **k: (lambda p: (p["split_k"], p["channels_per_workgroup"]))(ops.conv1d_plan(*a, **k))
    assert form(S12, 64, 64, P, fused_first=True) == (False, 64)
    for Ci, Co, L, S in ((64, 128, P, S12), (128, 256, P // 2, S12), (256, 512, P // 4, S34)):
        assert form(S, Ci, Co, L) == (False, 128), (Ci, Co, L)
    for Ci, Co in ((512, 256), (256, 128)):
        assert form(S34, Ci, Co, P // 8) == (False, 64), (Ci, Co)
    assert ops.spatial_attention_plan(B, N, 256 * (P // 4)) == (29, 29)
    torch.manual_seed(3)
    m = SpatialDROW(num_scans=T, num_pts=P, alpha=0.5, window_size=11, pedestrian_only=True).cuda().eval()
    gen = torch.Generator(device=DEV).manual_seed(5)
    x = torch.rand((B, N, T, P), generator=gen, device=DEV) - 0.5
    with torch.no_grad():
        ref = m(x)
        m.fuse_for_inference()
        got = m(x)
    for name, a, b in zip(("pred_cls", "pred_reg", "feat"), got, ref):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5, msg=lambda s, name=name: "%s: %s" % (name, s))


# ---------------------------------------------------------------- spatial attention segments
def _rows(B):
    """8 rows of a batch: first, last and six spread between them."""
    return sorted({0, B - 1} | {round(i * (B - 1) / 7) for i in range(1, 7)})


@pytest.mark.parametrize("B,N,fwd_seg,bwd_seg", ATTENTION_CASES)
def test_spatial_attention_segments(ops, B, N, fwd_seg, bwd_seg):
    """Forward merge and both backward forms at production batches (segments of 29 .. N points, a ragged last
    segment at N = 451) against autograd of the float64 torch formulation on 8 rows, at the bars of
    test_spatial_attention_backward_vs_autograd; the same rows bit-identical to B = 1 launches (short segments):
    every sum runs in a fixed order whatever the segment length."""
    E, Fd, w, alpha = ATTENTION_E, ATTENTION_F, ATTENTION_W, 0.5
    assert ops.spatial_attention_plan(B, N, Fd) == (fwd_seg, bwd_seg)
    assert ops.spatial_attention_plan(1, N, Fd)[0] <= 8
    gen = torch.Generator(device=DEV).manual_seed(B * 1000 + N)
    emb_x = torch.randn((B, N, E), generator=gen, device=DEV) * 0.3
    emb_t = torch.randn((B, N, E), generator=gen, device=DEV) * 0.3
    x = torch.randn((B, N, Fd), generator=gen, device=DEV)
    tmpl = torch.randn((B, N, Fd), generator=gen, device=DEV)
    out, band, prob = ops.spatial_attention(emb_x, emb_t, x, tmpl, alpha, w)
    rows = _rows(B)
    leaves = [t[rows].double().requires_grad_(True) for t in (emb_x, emb_t, x, tmpl)]
    out_r, band_r = _torch_attention(*leaves, alpha, w)
    torch.testing.assert_close(out[rows].double(), out_r.detach(), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(band[rows].double(), band_r.detach(), rtol=1e-4, atol=1e-5)
    for r in rows:
        one = ops.spatial_attention(emb_x[r:r + 1], emb_t[r:r + 1], x[r:r + 1], tmpl[r:r + 1], alpha, w)
        for name, a, b in zip(("out", "band", "prob"), one, (out, band, prob)):
            assert torch.equal(a, b[r:r + 1]), (name, r)
    del x, out
    g_out = torch.randn((B, N, Fd), generator=gen, device=DEV)
    g_band = torch.randn((B, N, band.shape[-1]), generator=gen, device=DEV)
    ((out_r * g_out[rows].double()).sum() + (band_r * g_band[rows].double()).sum()).backward()
    names = ("d_emb_x", "d_emb_t", "d_x", "d_tmpl")
    for fused in (True, False):
        grads = ops.spatial_attention_backward(emb_x, emb_t, tmpl, prob, g_out, g_band, alpha, w, fused=fused)
        for name, a, t in zip(names, grads, leaves):
            torch.testing.assert_close(a[rows].double(), t.grad, rtol=2e-4, atol=2e-4,
                                       msg=lambda s, name=name: "fused=%s %s: %s" % (fused, name, s))
        for r in rows:
            one = ops.spatial_attention_backward(emb_x[r:r + 1], emb_t[r:r + 1], tmpl[r:r + 1], prob[r:r + 1],
                                                 g_out[r:r + 1], g_band[r:r + 1], alpha, w, fused=fused)
            for name, a, b in zip(names, one, grads):
                assert torch.equal(a, b[r:r + 1]), ("fused=%s" % fused, name, r)
        del grads


# ---------------------------------------------------------------- training tail at the reference's batch
@pytest.mark.parametrize("S,groups,C,L,pool", BN_TAIL_CASES)
def test_bn_tail_at_training_batch(ops, S, groups, C, L, pool):
    """Fused BatchNorm(train) + LeakyReLU [+ pool] forward and backward with per-group statistics at the training
    batch (the per-chunk sequence caps of the statistics and element-wise passes are reached) against float64 torch,
    at the bars of test_fuzz_training_trunk_kernels."""
    slope = 0.1
    g = torch.Generator(device=DEV).manual_seed(S + groups)
    y = torch.randn((S, C, L), generator=g, device=DEV) * 1.7 + 0.3
    gam = torch.rand(C, generator=g, device=DEV) + 0.5
    bet = torch.rand(C, generator=g, device=DEV) - 0.5
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    z, mu, istd = ops.bn_lrelu_pool_forward(y, gam, bet, rm, rv, momentum=0.1, eps=1e-5, negative_slope=slope,
                                            pool=pool, groups=groups)
    y64 = y.double().requires_grad_(True)
    g64, b64 = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    rm64 = torch.zeros(C, device=DEV, dtype=torch.float64)
    rv64 = torch.ones(C, device=DEV, dtype=torch.float64)
    Sg = S // groups
    u = torch.cat([F.batch_norm(y64[i * Sg:(i + 1) * Sg], rm64, rv64, g64, b64, True, 0.1, 1e-5)
                   for i in range(groups)])                     # running statistics updated once per group, in order
    z64 = F.leaky_relu(u, slope)
    if pool:
        z64 = F.max_pool1d(z64, 2)
    assert torch.allclose(z.double(), z64, rtol=1e-5, atol=3e-5)
    assert torch.allclose(rv.double(), rv64, rtol=1e-5, atol=1e-6)
    assert torch.allclose(rm.double(), rm64, rtol=1e-5, atol=1e-6)
    dz = torch.randn(z.shape, generator=g, device=DEV)
    z64.backward(dz.double())
    del z, z64, u
    dy, dgam, dbet, dsum = ops.bn_lrelu_pool_backward(y, dz, gam, bet, mu, istd, negative_slope=slope, pool=pool,
                                                      bias_grad=True, groups=groups)
    # near a zero of u or a pooled tie the float32 forward may pick the other branch than float64 does: compare
    # where the float64 pre-activation is clear of both
    scale = max(float(y64.grad.abs().max()), 1e-3)
    bad = (dy.double() - y64.grad).abs() > 1e-4 * scale
    assert float(bad.double().mean()) < 2e-4
    # every element whose branch differs moves a per-channel sum by up to |dz| * |xhat| (gamma) or |dz| (beta)
    flips = float(bad.sum())
    y64 = y64.detach()
    xh_max = max(float(((yg - yg.mean(dim=(0, 2), keepdim=True)) / yg.std(dim=(0, 2), keepdim=True)).abs().max())
                 for yg in y64.split(Sg))
    dz_max = float(dz.abs().max())
    assert float((dgam.double() - g64.grad).abs().max()) <= 2e-3 * max(float(g64.grad.abs().max()), 1.0) \
        + 2.0 * flips * dz_max * xh_max
    assert float((dbet.double() - b64.grad).abs().max()) <= 2e-3 * max(float(b64.grad.abs().max()), 1.0) \
        + flips * dz_max
    assert float((dsum.double() - dy.double().sum(dim=(0, 2))).abs().max()) <= \
        1e-4 * max(float(dy.abs().sum(dim=(0, 2)).max()), 1.0)


def _wgrad_reference(x, dy):
    """float64 dL/dw of Conv1d(k = 3, padding 1): dw[co][ci][k] = sum over (s, l) of dy[s][co][l] x[s][ci][l + k - 1]."""
    S, Ci, L = x.shape
    Co = dy.shape[1]
    dw = torch.zeros((Co, Ci, 3), dtype=torch.float64, device=x.device)
    per = max(1, (1 << 24) // (max(Ci, Co) * L))
    for s0 in range(0, S, per):
        xs = F.pad(x[s0:s0 + per].double(), (1, 1))
        ds = dy[s0:s0 + per].double()
        for k in range(3):
            dw[:, :, k] += torch.einsum("scl,sdl->cd", ds, xs[:, :, k:k + L])
    return dw


@pytest.mark.parametrize("S,Ci,Co,L", WGRAD_CASES)
def test_conv3_wgrad_at_training_batch(ops, S, Ci, Co, L):
    """Split-K weight gradient at the training batch (hundreds of K splits): exact on integer data, 3e-5 relative
    on random data, against float64."""
    g = torch.Generator(device=DEV).manual_seed(S + Ci + Co + L)
    x = torch.randint(-2, 3, (S, Ci, L), generator=g, device=DEV, dtype=torch.int8).float()
    dy = torch.randint(-2, 3, (S, Co, L), generator=g, device=DEV, dtype=torch.int8).float()
    dw = ops.conv3_wgrad(x, dy)
    want = _wgrad_reference(x, dy)
    assert torch.equal(dw, want.float()), (dw.double() - want).abs().max().item()
    x = torch.randn((S, Ci, L), generator=g, device=DEV)
    dy = torch.randn((S, Co, L), generator=g, device=DEV)
    dw = ops.conv3_wgrad(x, dy)
    want = _wgrad_reference(x, dy)
    assert float((dw.double() - want).abs().max()) <= 3e-5 * max(float(want.abs().max()), 1.0)
