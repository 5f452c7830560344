"""Float16 activation STORAGE through the DR-SPAAM inference path: pof_conv3_bn_lrelu_f16,
pof_conv3_first_two_f16, pof_drow_heads_f16 and ``fuse_for_inference(storage=torch.float16)``.

Every product and sum stays float32, in the order of the float32 kernel of the same shape, and a float16 widens to
float32 exactly.  So the contract is equality, bit for bit, with the float32 kernel on the widened values, rounded once:
every comparison below is ``torch.equal``; there is no tolerance.  Each conv case first asserts, through the host-only
plan query, the kernel form it is there for.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
F16_MIN_NORMAL = 2.0 ** -14
F16_MAX = 65504.0


@pytest.fixture(scope="module")
def ops():
    from planar_optical_flow_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _ops


@pytest.fixture(autouse=True)
def _release_memory():
    yield
    torch.cuda.empty_cache()


def _layer(gen, Ci, Co):
    wt = (torch.randn((3, Ci, Co), generator=gen, device=DEV) / (3 * Ci) ** 0.5).contiguous()
    scale = torch.rand((Co,), generator=gen, device=DEV) + 0.5
    shift = torch.randn((Co,), generator=gen, device=DEV)
    return wt, scale, shift


# ---------------------------------------------------------------- 1. the layer, every form
# (S, Ci, Co, L, pool, negative_slope, split_k, channels per workgroup).  Tails covered: Ci = 5 / 7 (partial chunk,
# missing odd channel of a pair), Co = 33 / 6 (partial tile, not a multiple of 4), L = 7 unpooled, L = 14 and 56
# pooled, S * L not a multiple of 32 (35, 42, 32662, 262024, 56, 63, 126), slopes 0.1 and 1.5 / -0.25.
LAYER_CASES = [
    (5, 5, 33, 7, False, 0.1, False, 32),
    (3, 7, 6, 14, True, 1.5, False, 32),
    (2333, 7, 64, 14, True, 0.1, False, 64),        # 256 workgroups of 64 channels
    (4679, 8, 128, 56, True, -0.25, False, 128),    # 2048 workgroups of 128 channels
    (8, 128, 64, 7, False, 0.1, True, 32),
    (9, 512, 256, 7, False, 0.1, True, 64),
    (9, 130, 40, 14, True, 1.5, True, 32),          # split K with a partial last chunk and a partial channel tile
]


@pytest.mark.parametrize("case", LAYER_CASES, ids=lambda c: "S%d-%dx%d-L%d%s-%s%d" % (
    c[0], c[1], c[2], c[3], "-pool" if c[4] else "", "splitk" if c[6] else "ct", c[7]))
def test_layer_equals_float32_layer_rounded_once(ops, case):
    S, Ci, Co, L, pool, slope, split, cpw = case
    plan = ops.conv1d_plan(S, Ci, Co, L, 3, 1, pool)
    assert plan == dict(split_k=split, channels_per_workgroup=cpw, launches=1, wide_offsets=0), plan
    gen = torch.Generator(device=DEV).manual_seed(S * 7 + Ci * 131 + Co + L)
    x16 = torch.randn((S, Ci, L), generator=gen, device=DEV).half()
    wt, scale, shift = _layer(gen, Ci, Co)
    got = ops.conv3_bn_lrelu(x16, wt, scale, shift, pool=pool, negative_slope=slope)
    want = ops.conv3_bn_lrelu(x16.float(), wt, scale, shift, pool=pool, negative_slope=slope)
    assert got.dtype == torch.float16 and got.shape == want.shape
    assert torch.isfinite(want).all()
    assert torch.equal(got, want.half())


def test_registered_operator_keeps_the_storage_type(ops):
    gen = torch.Generator(device=DEV).manual_seed(3)
    x16 = torch.randn((4, 6, 10), generator=gen, device=DEV).half()
    wt, scale, shift = _layer(gen, 6, 8)
    got = torch.ops.pof.conv3_bn_lrelu(x16, wt, scale, shift, True, 0.1)
    assert got.dtype == torch.float16
    assert torch.equal(got, ops.conv3_bn_lrelu(x16.float(), wt, scale, shift, pool=True).half())
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        z = torch.ops.pof.conv3_bn_lrelu(torch.empty(7, 64, 56, device=DEV, dtype=torch.float16),
                                         torch.empty(3, 64, 128, device=DEV), torch.empty(128, device=DEV),
                                         torch.empty(128, device=DEV), True, 0.1)
        assert tuple(z.shape) == (7, 128, 28) and z.dtype == torch.float16


# ---------------------------------------------------------------- 2. the first two units in one launch
# (S, C1, Co, L, pool, channels per workgroup)
FIRST_TWO_CASES = [
    (3, 64, 64, 56, False, 32),
    (3, 64, 64, 56, True, 32),
    (5, 6, 40, 10, True, 32),          # ragged: partial chunk, partial tile, S * L = 50
    (600, 64, 64, 56, True, 64),       # the 64- and 128-channel instantiations of the fused form
    (4679, 8, 128, 56, True, 128),
]


@pytest.mark.parametrize("case", FIRST_TWO_CASES, ids=lambda c: "S%d-%dx%d-L%d%s-ct%d" % (
    c[0], c[1], c[2], c[3], "-pool" if c[4] else "", c[5]))
def test_first_two_equals_float32_call_rounded_once(ops, case):
    S, C1, Co, L, pool, cpw = case
    plan = ops.conv1d_plan(S, C1, Co, L, 3, 1, pool, fused_first=True)
    assert plan == dict(split_k=False, channels_per_workgroup=cpw, launches=1, wide_offsets=0), plan
    gen = torch.Generator(device=DEV).manual_seed(S + C1 * 17 + Co + L)
    x16 = (torch.randn((S, L), generator=gen, device=DEV) * 3).half()
    table = torch.cat((torch.randn((C1, 3), generator=gen, device=DEV) * 0.5,
                       torch.randn((C1, 1), generator=gen, device=DEV) * 0.2), dim=1).contiguous()
    wt, scale, shift = _layer(gen, C1, Co)
    got = ops.conv3_first_two(x16, table, wt, scale, shift, slope1=0.1, pool=pool, negative_slope=0.1)
    want = ops.conv3_first_two(x16.float(), table, wt, scale, shift, slope1=0.1, pool=pool, negative_slope=0.1)
    assert got.dtype == torch.float16 and got.shape == want.shape
    assert torch.equal(got, want.half())
    # [S, 1, L] is the same call
    assert torch.equal(ops.conv3_first_two(x16[:, None, :], table, wt, scale, shift, pool=pool), got)


# ---------------------------------------------------------------- 3. rounding edges
def test_rounding_edges_subnormals_and_overflow(ops):
    """Float16 subnormals on input, outputs in the float16 subnormal range and outputs beyond 65504: all equal to
    .half() of the float32 result (round to nearest even, no flush, +-inf on overflow)."""
    S, Ci, Co, L = 4, 8, 32, 14
    gen = torch.Generator(device=DEV).manual_seed(11)
    wt, scale, shift = _layer(gen, Ci, Co)
    zero = torch.zeros_like(shift)
    x16 = torch.randn((S, Ci, L), generator=gen, device=DEV).half()

    # subnormal inputs (|x| < 2^-14, non-zero); unit scale, so that they reach the output
    xs = (torch.randn((S, Ci, L), generator=gen, device=DEV) * 1e-4).half()
    sub_in = (xs != 0) & (xs.abs().float() < F16_MIN_NORMAL)
    assert sub_in.any() and not sub_in.all() and not torch.isnan(xs).any()
    want = ops.conv3_bn_lrelu(xs.float(), wt, torch.ones_like(scale), zero)
    assert (want != 0).any()
    assert torch.equal(ops.conv3_bn_lrelu(xs, wt, torch.ones_like(scale), zero), want.half())

    # part of the output in the float16 subnormal range
    want = ops.conv3_bn_lrelu(x16.float(), wt, scale * 2e-5, zero)
    sub_out = (want != 0) & (want.abs() < F16_MIN_NORMAL)
    assert sub_out.any() and (want.abs() >= 2.0 ** -24).any()
    got = ops.conv3_bn_lrelu(x16, wt, scale * 2e-5, zero)
    assert torch.equal(got, want.half())
    assert ((got != 0) & (got.abs().float() < F16_MIN_NORMAL)).any()          # really kept, not flushed

    # outputs beyond the float16 range, pooled and unpooled, both signs (slope 1.5 keeps the negatives large)
    for pool in (False, True):
        want = ops.conv3_bn_lrelu(x16.float(), wt, scale * 1e5, shift, pool=pool, negative_slope=1.5)
        assert torch.isfinite(want).all()
        assert (want > F16_MAX).any() and (want.abs() < F16_MAX).any()
        assert pool or (want < -F16_MAX).any()
        got = ops.conv3_bn_lrelu(x16, wt, scale * 1e5, shift, pool=pool, negative_slope=1.5)
        assert torch.isinf(got).any() and not torch.isnan(got).any()
        assert torch.equal(got, want.half())


# ---------------------------------------------------------------- 4. pointer offsets
@pytest.mark.parametrize("pool", [False, True])
def test_layer_at_odd_element_offsets(ops, pool):
    """x and out carved at odd float16 element offsets (2-byte alignment only) of larger buffers: the bits of the
    aligned call, and nothing written outside out."""
    S, Ci, Co, L = 5, 7, 33, 14
    gen = torch.Generator(device=DEV).manual_seed(21)
    x16 = torch.randn((S, Ci, L), generator=gen, device=DEV).half()
    wt, scale, shift = _layer(gen, Ci, Co)
    ref = ops.conv3_bn_lrelu(x16, wt, scale, shift, pool=pool)
    n_out = ref.numel()
    for kx, ko in ((1, 0), (0, 1), (3, 5), (7, 1)):
        xbuf = torch.zeros(x16.numel() + 16, dtype=torch.float16, device=DEV)
        xbuf[kx:kx + x16.numel()] = x16.reshape(-1)
        obuf = torch.full((n_out + 16,), -7.0, dtype=torch.float16, device=DEV)
        xv = xbuf[kx:kx + x16.numel()].view(S, Ci, L)
        ov = obuf[ko:ko + n_out].view(ref.shape)
        assert xv.data_ptr() % 4 == 2 * (kx % 2) and ov.data_ptr() % 4 == 2 * (ko % 2)
        ops.conv3_bn_lrelu(xv, wt, scale, shift, pool=pool, out=ov)
        assert torch.equal(ov, ref), (kx, ko)
        assert (obuf[:ko] == -7).all() and (obuf[ko + n_out:] == -7).all(), (kx, ko)


def test_first_two_at_odd_element_offsets(ops):
    S, C1, Co, L = 5, 6, 40, 10
    gen = torch.Generator(device=DEV).manual_seed(22)
    x16 = torch.randn((S, L), generator=gen, device=DEV).half()
    table = torch.randn((C1, 4), generator=gen, device=DEV) * 0.5
    wt, scale, shift = _layer(gen, C1, Co)
    ref = ops.conv3_first_two(x16, table, wt, scale, shift)
    xbuf = torch.zeros(x16.numel() + 4, dtype=torch.float16, device=DEV)
    xbuf[1:1 + x16.numel()] = x16.reshape(-1)
    obuf = torch.full((ref.numel() + 4,), -7.0, dtype=torch.float16, device=DEV)
    ov = obuf[3:3 + ref.numel()].view(ref.shape)
    ops.conv3_first_two(xbuf[1:1 + x16.numel()].view(S, L), table, wt, scale, shift, out=ov)
    assert torch.equal(ov, ref)
    assert (obuf[:3] == -7).all() and (obuf[3 + ref.numel():] == -7).all()


# ---------------------------------------------------------------- 5. heads
@pytest.mark.parametrize("n_cls", [1, 4])
@pytest.mark.parametrize("L", [7, 1])
def test_heads_read_float16(ops, n_cls, L):
    S, C = 37, 128
    gen = torch.Generator(device=DEV).manual_seed(31 + n_cls + L)
    feat16 = torch.randn((S, C, L), generator=gen, device=DEV).half()
    wc, bc = torch.randn((n_cls, C), generator=gen, device=DEV), torch.randn((n_cls,), generator=gen, device=DEV)
    wr, br = torch.randn((2, C), generator=gen, device=DEV), torch.randn((2,), generator=gen, device=DEV)
    cls16, reg16 = ops.drow_heads(feat16, wc, bc, wr, br)
    cls32, reg32 = ops.drow_heads(feat16.float(), wc, bc, wr, br)
    assert cls16.dtype == reg16.dtype == torch.float32
    assert torch.equal(cls16, cls32) and torch.equal(reg16, reg32)
    assert (cls32 != 0).all()
    # feat one element off a 4-byte boundary
    buf = torch.zeros(feat16.numel() + 2, dtype=torch.float16, device=DEV)
    buf[1:-1] = feat16.reshape(-1)
    cls_o, reg_o = ops.drow_heads(buf[1:-1].view(S, C, L), wc, bc, wr, br)
    assert torch.equal(cls_o, cls32) and torch.equal(reg_o, reg32)


# ---------------------------------------------------------------- 6. the model
B, N, T, P = 1, 40, 3, 48


def _seeded_model(cls):
    """Seeded construction, BatchNorm running statistics and affine parameters randomised (a fresh model's are 0 / 1,
    which would hide a wrong fold)."""
    from planar_optical_flow_amd.src.depracted.model import dr_spaam
    torch.manual_seed(1234)
    kw = dict(window_size=7) if cls == "SpatialDROW" else {}
    model = getattr(dr_spaam, cls)(num_pts=P, **kw)
    gen = torch.Generator().manual_seed(99)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            with torch.no_grad():
                m.running_mean.copy_(torch.randn(m.num_features, generator=gen) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=gen) + 0.5)
                m.weight.copy_(torch.rand(m.num_features, generator=gen) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=gen) * 0.1)
    return model.cuda().eval()


def _cutouts(seed, t):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn((B, N, t, P), generator=gen, device=DEV) * 2).half()


class _Chain:
    """The float16-storage forward written out from the FLOAT32 ops, with an explicit .half() at every stored tensor."""

    def __init__(self, ops, model):
        self.ops, self.m, self.f = ops, model, model._fused

    def block(self, name, h, pool):
        layers, start = self.f[name], 0
        if name == "conv_block_1":
            wt, sc, sh = layers[1]
            h = self.ops.conv3_first_two(h.float(), self.f["first_unit_table"], wt, sc, sh, slope1=0.1, pool=False,
                                         negative_slope=0.1).half()
            start = 2
        for i in range(start, len(layers)):
            wt, sc, sh = layers[i]
            h = self.ops.conv3_bn_lrelu(h.float(), wt, sc, sh, pool=pool and i == len(layers) - 1).half()
        return h

    def scan_features(self, seqs16):
        """[S, P] float16 cutouts -> [S, 256, P / 4] float16"""
        return self.block("conv_block_2", self.block("conv_block_1", seqs16, True), True)

    def gate(self, x16, t16):
        gate = self.m.gate
        flat = B * N, x16.shape[-2] * x16.shape[-1]
        emb_x = gate._embed_rows(x16.reshape(flat)).view(B, N, 128)
        emb_t = gate._embed_rows(t16.reshape(flat)).view(B, N, 128)
        out, band, _ = self.ops.spatial_attention(emb_x, emb_t, x16.float().contiguous(), t16.float().contiguous(),
                                                  gate._alpha, gate._window_size)
        return out.half(), band

    def heads(self, tmpl16):
        h = self.block("conv_block_3", tmpl16.reshape((B * N,) + tuple(tmpl16.shape[-2:])), True)
        h = self.block("conv_block_4", h, False)
        m = self.m
        cls, reg = self.ops.drow_heads(h.float(), m.conv_cls.weight, m.conv_cls.bias, m.conv_reg.weight, m.conv_reg.bias)
        return cls.view(B, N, -1), reg.view(B, N, 2)


@pytest.fixture(scope="module")
def spatial_model():
    return _seeded_model("SpatialDROW")


def test_spatial_drow_equals_the_float32_ops_with_explicit_rounding(ops, spatial_model, capsys):
    model = spatial_model.fuse_for_inference(storage=torch.float16)
    x16 = _cutouts(5, T)
    with torch.no_grad():
        got = model(x16)
        again = model(x16.float())
        chain = _Chain(ops, model)
        feats = chain.scan_features(x16.permute(2, 0, 1, 3).reshape(T * B * N, P))      # scan-major, as the model
        feats = feats.view(T, B, N, feats.shape[-2], feats.shape[-1])
        tmpl = feats[0]
        for t in range(1, T):
            tmpl, band = chain.gate(feats[t], tmpl)
        want = chain.heads(tmpl) + (band,)
    assert all(g.dtype == torch.float32 for g in got)
    for g, a, w in zip(got, again, want):
        assert g.shape == w.shape and torch.isfinite(w).all()
        assert torch.equal(g, w)
        assert torch.equal(g, a)                     # float16 cutout == float32 cutout of the same values
    # the cost of float16 storage against float32 storage: a record, not a bar
    with torch.no_grad():
        model.fuse_for_inference()
        ref = model(x16.float())
    assert all(r.dtype == torch.float32 and torch.isfinite(r).all() for r in ref)
    with capsys.disabled():
        print("\nfloat16 storage vs float32 storage, max |difference| (at max |float32|): "
              + ", ".join("%s %.3e (%.3e)" % (n, (g - r).abs().max().item(), r.abs().max().item())
                          for n, g, r in zip(("pred_cls", "pred_reg", "feat_fused"), got, ref)))


def test_spatial_drow_streaming_form_over_three_calls(ops, spatial_model):
    model = spatial_model.fuse_for_inference(storage=torch.float16)
    chain = _Chain(ops, model)
    tmpl_m = tmpl_m32 = tmpl_c = None
    with torch.no_grad():
        for call in range(3):
            x16 = _cutouts(40 + call, 1)
            cls, reg, tmpl_m, fused = model(x16, testing=True, fea_template=tmpl_m)
            cls32, reg32, tmpl_m32, fused32 = model(x16.float(), testing=True, fea_template=tmpl_m32)
            feat = chain.scan_features(x16.reshape(B * N, P)).view(B, N, 256, P // 4)
            if tmpl_c is None:
                tmpl_c = feat.clone()
                _, band = chain.gate(feat, tmpl_c)
            else:
                tmpl_c, band = chain.gate(feat, tmpl_c)
            wcls, wreg = chain.heads(tmpl_c)
            assert tmpl_m.dtype == torch.float16 and cls.dtype == reg.dtype == fused.dtype == torch.float32
            for g, a, w in ((cls, cls32, wcls), (reg, reg32, wreg), (tmpl_m, tmpl_m32, tmpl_c), (fused, fused32, band)):
                assert torch.equal(g, w), call
                assert torch.equal(g, a), call
    assert not torch.equal(tmpl_c, feat)             # the template really was carried and merged


def test_plain_drow_float16_storage(ops):
    model = _seeded_model("DROW").fuse_for_inference(storage=torch.float16)
    x16 = _cutouts(6, T)
    with torch.no_grad():
        got = model(x16)
        again = model(x16.float())
        chain = _Chain(ops, model)
        feats = chain.scan_features(x16.reshape(B * N * T, P))                           # cutout-major, as the model
        feats = feats.view(B, N, T, feats.shape[-2], feats.shape[-1])
        want = chain.heads(torch.sum(feats, dim=2, dtype=torch.float32).half())
    for g, a, w in zip(got, again, want):
        assert g.dtype == torch.float32 and torch.equal(g, w) and torch.equal(g, a)
    model.train()
    assert model._fused is None and model._storage == torch.float32


# ---------------------------------------------------------------- 7. refusals and defaults
def test_refusals(ops, spatial_model):
    from planar_optical_flow_amd.streaming import StreamingDetector
    model = spatial_model.fuse_for_inference(storage=torch.float16)
    with pytest.raises(ValueError):
        StreamingDetector(model, num_pts=N)
    with pytest.raises(ValueError):
        model.fuse_for_inference(storage=torch.bfloat16)
    gen = torch.Generator(device=DEV).manual_seed(1)
    wt, scale, shift = _layer(gen, 4, 8)
    x16 = torch.zeros((2, 4, 8), dtype=torch.float16, device=DEV)
    with pytest.raises(TypeError):
        ops.conv1d_bn_lrelu(x16, wt, scale, shift)
    with pytest.raises(TypeError):
        ops.conv3_bn_lrelu(x16.cpu(), wt, scale, shift)
    with pytest.raises(TypeError):
        ops.conv3_first_two(x16[:, 0].cpu(), torch.zeros((4, 4), device=DEV), wt, scale, shift)
    with pytest.raises(TypeError):
        ops.drow_heads(x16.cpu(), wt[0].t().contiguous()[:1], scale[:1], wt[0].t().contiguous()[:2], scale[:2])
    with pytest.raises(TypeError):                   # no mixed in / out form
        ops.conv3_bn_lrelu(x16, wt, scale, shift, out=torch.empty((2, 8, 8), device=DEV))
    with pytest.raises(TypeError):
        ops.conv3_bn_lrelu(x16.to(torch.bfloat16), wt, scale, shift)
    # the default stays float32 storage
    model.fuse_for_inference()
    assert model._storage == torch.float32 and model.gate._storage == torch.float32
    with torch.no_grad():
        out = model(_cutouts(7, T), testing=False)
    assert all(o.dtype == torch.float32 for o in out)
    StreamingDetector(model, num_pts=N)
