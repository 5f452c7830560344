"""The attention gate's embedding on the HIP kernel: pof_attn_embed / pof_attn_embed_f16,
``ops.attn_embed``, ``fuse_for_inference(embed="hip")`` and the float16 streaming detector.

The kernel owns its summation order (include/pof_abi.h): 8-element k-chunks dealt round-robin onto four chains, inside a
chunk k = 8c + {0, 4, 1, 5, 2, 6, 3, 7}, every step one fmaf; ((p0 + p1) + p2) + p3, + bias, LeakyReLU.  A host referee
walks that order with libm's fmaf and the kernel has to give its bits; on integer data the result is exact; a row's
result depends on that row only, whatever the batch, the slot, the storage type and the kernel form.
"""
import contextlib
import ctypes
import ctypes.util

import numpy as np
import pytest
import torch

from planar_optical_flow_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
LARGE = 8192             # rows from which pof_attn_embed_plan reports form 1


@pytest.fixture(scope="module")
def ops():
    from planar_optical_flow_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert _ops.attn_embed_plan(LARGE - 1, 8, 32) == 0 and _ops.attn_embed_plan(LARGE, 8, 32) == 1
    return _ops


@pytest.fixture(autouse=True)
def _release_memory():
    yield
    torch.cuda.empty_cache()


def _normal(gen, *shape):
    return torch.randn(shape, generator=gen, device=DEV)


def _problem(seed, R, K, E, two=True):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x = _normal(gen, R, K)
    t = _normal(gen, R, K) if two else None
    w = (_normal(gen, E, K) / K ** 0.5).contiguous()
    b = _normal(gen, E) * 0.3
    return x, t, w, b


# ---------------------------------------------------------------- 1. bits against a host referee
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_float]


def _referee_row(xrow, w, bias, slope):
    """The documented order, one row against every channel, with libm's fmaf."""
    K, f32, fmaf = xrow.shape[0], np.float32, _libm.fmaf
    order = [(c % 4, 8 * c + o) for c in range(K // 8) for o in (0, 4, 1, 5, 2, 6, 3, 7)]
    xs = [float(v) for v in xrow]
    out = np.empty(w.shape[0], dtype=np.float32)
    for e in range(w.shape[0]):
        we = [float(v) for v in w[e]]
        p = [0.0, 0.0, 0.0, 0.0]
        for q, k in order:
            p[q] = fmaf(xs[k], we[k], p[q])
        s = f32(f32(f32(f32(p[0]) + f32(p[1])) + f32(p[2])) + f32(p[3]))
        v = f32(s + f32(bias[e]))
        out[e] = v if v >= 0 else f32(v * f32(slope))
    return out


@pytest.mark.parametrize("K,rows", [(512, ((0, 0), (0, 33), (0, 69), (1, 0), (1, 33), (1, 69))),
                                    (3584, ((0, 7), (1, 69)))], ids=["K512", "K3584"])
def test_bits_equal_the_host_referee(ops, K, rows):
    """R = 70, E = 128, random normal data; (slot, row) pairs checked over all 128 channels."""
    x, t, w, b = _problem(K, 70, K, 128)
    emb = ops.attn_embed(x, t, w, b, 0.1)
    assert emb[0].shape == emb[1].shape == (70, 128) and emb[0].dtype == torch.float32
    src, wn, bn = (x.cpu().numpy(), t.cpu().numpy()), w.cpu().numpy(), b.cpu().numpy()
    for slot, row in rows:
        want = torch.from_numpy(_referee_row(src[slot][row], wn, bn, 0.1))
        got = emb[slot][row].cpu()
        assert (want < 0).any() and (want > 0).any()
        assert torch.equal(got, want), (slot, row, (got - want).abs().max().item())


# ---------------------------------------------------------------- 2. exact on integer data
# (R, K, E, two sources).  R: 1, tile edges 31 / 32 / 33 / 63 / 65 / 129, the streaming 450, 907, both sides of the form
# boundary (8191: last of form 0, 8192: smallest of form 1, 8225: form 1 with a ragged last tile pair).  K: one chunk
# (8), a ragged chain split (40 = 5 chunks), 512, 3072, 3584.  E: 32, 128, 256 (and 64, 96: spare waves of form 1).
INT_CASES = [
    (1, 8, 32, False), (31, 512, 128, True), (32, 3072, 256, True), (33, 8, 128, True), (63, 3584, 32, True),
    (65, 512, 256, False), (129, 3072, 128, True), (450, 3584, 128, True), (907, 512, 32, True), (70, 40, 64, True),
    (8191, 8, 128, True), (8192, 512, 128, True), (8225, 40, 256, True), (8192, 3584, 128, False), (8200, 8, 96, True),
]


@pytest.mark.parametrize("case", INT_CASES, ids=lambda c: "R%d-K%d-E%d-%s" % (c[0], c[1], c[2], "two" if c[3] else "one"))
def test_exact_on_integer_data(ops, case):
    """x in [-4, 4], w in [-3, 3], integer bias: every partial sum is an integer below 2^24 (3584 * 12 + 8), so every
    float32 order gives the float64 product exactly.  Slope 0.5 is exact as well; slope 0.1 is one float32 multiply."""
    R, K, E, two = case
    assert ops.attn_embed_plan(R, K, E) == (1 if R >= LARGE else 0)
    gen = torch.Generator(device=DEV).manual_seed(R * 31 + K + E)
    x = torch.randint(-4, 5, (R, K), generator=gen, device=DEV).float()
    t = torch.randint(-4, 5, (R, K), generator=gen, device=DEV).float() if two else None
    w = torch.randint(-3, 4, (E, K), generator=gen, device=DEV).float()
    b = torch.randint(-8, 9, (E,), generator=gen, device=DEV).float()
    pre = [(s.double() @ w.double().t() + b.double()).float() for s in ((x, t) if two else (x,))]
    for slope in (0.5, 0.1):
        emb = ops.attn_embed(x, t, w, b, slope)
        assert emb[1] is None or two
        for got, v in zip(emb, pre):
            want = torch.where(v >= 0, v, v * torch.tensor(slope, dtype=torch.float32, device=DEV))
            assert got.shape == (R, E) and torch.equal(got, want), (slope, (got - want).abs().max().item())
    assert (pre[0] < 0).any() and (pre[0] > 0).any()


# ---------------------------------------------------------------- 3. a-priori bound on random data
@pytest.mark.parametrize("R,K", [(70, 3584), (LARGE + 8, 512)], ids=["form0", "form1"])
def test_within_the_a_priori_float32_bound(ops, R, K, capsys):
    """|err| <= (K + 3) * 2^-24 * (sum_k |x w| + |bias|) against the float64 product: holds for ANY float32 summation
    order of K products, three chain additions and the bias (a gross-error check; the referee test is the sharp one).
    Slope 1 keeps the pre-activation value."""
    x, t, w, b = _problem(3 + R, R, K, 128)
    emb = ops.attn_embed(x, t, w, b, 1.0)
    worst = 0.0
    for got, s in zip(emb, (x, t)):
        ref = s.double() @ w.double().t() + b.double()
        mag = s.double().abs() @ w.double().abs().t() + b.double().abs()
        ratio = ((got.double() - ref).abs() / ((K + 3) * 2.0 ** -24 * mag)).max().item()
        worst = max(worst, ratio)
    with capsys.disabled():
        print("\nattn_embed R=%d K=%d: largest |err| / bound = %.4f" % (R, K, worst))
    assert worst <= 1.0


# ---------------------------------------------------------------- 4. a row's result depends on that row only
def test_row_results_do_not_depend_on_the_batch(ops):
    x, t, w, b = _problem(17, 70, 512, 128)
    ex, et = ops.attn_embed(x, t, w, b, 0.1)
    for i in (0, 40, 69):                             # first tile, a middle tile, the ragged last tile
        one = ops.attn_embed(x[i:i + 1], None, w, b, 0.1)[0]
        assert torch.equal(one[0], ex[i]), i
    perm = torch.randperm(70, generator=torch.Generator().manual_seed(5)).to(DEV)
    px, pt = ops.attn_embed(x[perm].contiguous(), t[perm].contiguous(), w, b, 0.1)
    assert torch.equal(px, ex[perm]) and torch.equal(pt, et[perm])
    # the template slot gives the bits of the x slot for the same rows
    sx, st = ops.attn_embed(t, x, w, b, 0.1)
    assert torch.equal(sx, et) and torch.equal(st, ex)
    assert torch.equal(ops.attn_embed(t, None, w, b, 0.1)[0], et)


@pytest.mark.parametrize("K", [3584, 40], ids=["K3584", "K40"])
def test_both_sides_of_the_form_boundary_give_equal_rows(ops, K):
    x, t, w, b = _problem(23 + K, LARGE + 40, K, 128)
    assert ops.attn_embed_plan(LARGE - 1, K, 128) == 0 and ops.attn_embed_plan(LARGE, K, 128) == 1
    below = ops.attn_embed(x[:LARGE - 1], t[:LARGE - 1], w, b, 0.1)              # form 0
    at = ops.attn_embed(x[:LARGE], t[:LARGE], w, b, 0.1)                          # form 1, the smallest
    above = ops.attn_embed(x, t, w, b, 0.1)                                      # form 1, ragged last workgroup
    small = ops.attn_embed(x[LARGE - 30:], t[LARGE - 30:], w, b, 0.1)            # form 0 on the rows around the boundary
    for s in (0, 1):
        assert torch.equal(below[s], at[s][:LARGE - 1]) and torch.equal(at[s], above[s][:LARGE])
        assert torch.equal(small[s], above[s][LARGE - 30:])


# ---------------------------------------------------------------- 5. float16 storage
@pytest.mark.parametrize("R,K", [(70, 512), (LARGE + 8, 40)], ids=["form0", "form1"])
def test_float16_rows_give_the_bits_of_the_widened_rows(ops, R, K):
    x, t, w, b = _problem(29 + R, R, K, 128)
    x16, t16 = x.half(), (t * 1e-4).half()
    sub = (t16 != 0) & (t16.abs().float() < 2.0 ** -14)
    assert sub.any() and not sub.all()                               # float16 subnormals among the rows
    x16[0, :8] = torch.tensor([65504.0, -65504.0, 2.0 ** -24, -2.0 ** -24, 65504.0, 0.0, -0.0, 2.0 ** -14], device=DEV).half()
    x16[R - 1, K - 4:] = torch.tensor([-65504.0, 65504.0, 6e-8, -6e-8], device=DEV).half()
    got = ops.attn_embed(x16, t16, w, b, 0.1)
    want = ops.attn_embed(x16.float(), t16.float(), w, b, 0.1)
    assert all(g.dtype == torch.float32 and torch.isfinite(g).all() for g in got)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert (got[1] != 0).all()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_rows_and_weights_at_element_offsets(ops, dtype):
    """Views 16 bytes into a buffer (aligned for the kernel, not for a 256-byte allocation) go to the kernel as they are;
    views one element in are not 16-byte aligned and go through the wrapper's copy.  Same bits."""
    R, K, E = 70, 512, 128
    x, t, w, b = _problem(31, R, K, E)
    x, t = x.to(dtype), t.to(dtype)
    ref = ops.attn_embed(x, t, w, b, 0.1)
    per16 = 16 // x.element_size()
    for off in (per16, 1, per16 + 1):
        bufs = [torch.zeros(R * K + 2 * per16, dtype=dtype, device=DEV) for _ in range(2)]
        views = []
        for buf, s in zip(bufs, (x, t)):
            buf[off:off + R * K] = s.reshape(-1)
            views.append(buf[off:off + R * K].view(R, K))
        assert (views[0].data_ptr() % 16 == 0) == (off == per16) and views[0].data_ptr() % 256 != 0
        wbuf = torch.zeros(E * K + 8, device=DEV)
        wbuf[off % 4 + 4 * (off // per16):][:E * K] = w.reshape(-1)
        wv = wbuf[off % 4 + 4 * (off // per16):][:E * K].view(E, K)
        got = ops.attn_embed(views[0], views[1], wv, b, 0.1)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), off


def test_registered_operator_is_one_node(ops):
    from planar_optical_flow_amd import torch_ops  # noqa: F401  (registers torch.ops.pof.*)
    x, t, w, b = _problem(37, 33, 64, 32)
    ex, et = torch.ops.pof.attn_embed(x, t, w, b, 0.1)
    want = ops.attn_embed(x, t, w, b, 0.1)
    assert torch.equal(ex, want[0]) and torch.equal(et, want[1])
    ex1, et1 = torch.ops.pof.attn_embed(x.half(), None, w, b, 0.1)
    assert torch.equal(ex1, ops.attn_embed(x.half(), None, w, b, 0.1)[0]) and et1.shape == (0, 32)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        fx, ft = torch.ops.pof.attn_embed(torch.empty(450, 3584, device=DEV, dtype=torch.float16),
                                          torch.empty(450, 3584, device=DEV, dtype=torch.float16),
                                          torch.empty(128, 3584, device=DEV), torch.empty(128, device=DEV), 0.1)
        assert fx.shape == ft.shape == (450, 128) and fx.dtype == ft.dtype == torch.float32


# ---------------------------------------------------------------- 6. refusals
def test_refusals(ops):
    from planar_optical_flow_amd import _lib
    x, t, w, b = _problem(41, 4, 16, 32)
    with pytest.raises(TypeError):
        ops.attn_embed(x.cpu(), None, w, b, 0.1)
    with pytest.raises(TypeError):
        ops.attn_embed(x, t.cpu(), w, b, 0.1)
    with pytest.raises(TypeError):
        ops.attn_embed(x.to(torch.bfloat16), None, w, b, 0.1)
    with pytest.raises(TypeError):
        ops.attn_embed(x, t.half(), w, b, 0.1)                      # mixed storage types
    with pytest.raises(TypeError):
        ops.attn_embed(x.half(), t, w, b, 0.1)
    with pytest.raises(TypeError):
        ops.attn_embed(x, t, w.half(), b, 0.1)
    with pytest.raises(ValueError):
        ops.attn_embed(x[:, :12].contiguous(), None, w[:, :12].contiguous(), b, 0.1)      # K % 8 != 0
    with pytest.raises(ValueError):
        ops.attn_embed(x, None, torch.zeros(48, 16, device=DEV), torch.zeros(48, device=DEV), 0.1)    # E = 48
    with pytest.raises(ValueError):
        ops.attn_embed(x[:0], None, w, b, 0.1)                      # R = 0
    with pytest.raises(ValueError):
        ops.attn_embed(x, t[:3], w, b, 0.1)
    # the library itself, without the wrapper's checks: shape and alignment are refused before any launch
    lib, p = _lib.load(), lambda v: ctypes.c_void_p(v.data_ptr())
    out = torch.full((4, 32), -7.0, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.pof_attn_embed(p(x), None, 4, 12, 32, p(w), p(b), 0.1, p(out), None, stream) == _lib.POF_E_SHAPE
    assert lib.pof_attn_embed(p(x), None, 4, 16, 48, p(w), p(b), 0.1, p(out), None, stream) == _lib.POF_E_SHAPE
    assert lib.pof_attn_embed(p(x), None, 0, 16, 32, p(w), p(b), 0.1, p(out), None, stream) == _lib.POF_E_BADARG
    assert lib.pof_attn_embed(p(x), p(t), 4, 16, 32, p(w), p(b), 0.1, p(out), None, stream) == _lib.POF_E_BADARG
    assert lib.pof_attn_embed(ctypes.c_void_p(x.data_ptr() + 4), None, 3, 16, 32, p(w), p(b), 0.1, p(out), None,
                              stream) == _lib.POF_E_SHAPE
    assert lib.pof_attn_embed_f16(ctypes.c_void_p(x.data_ptr() + 8), None, 3, 16, 32, p(w), p(b), 0.1, p(out), None,
                                  stream) == _lib.POF_E_SHAPE
    torch.cuda.synchronize()
    assert (out == -7).all()


# ---------------------------------------------------------------- 7. the model against the reference's numbers
def test_spatial_drow_with_hip_embedding_equals_reference(golden, capsys):
    from planar_optical_flow_amd.src.depracted.model.dr_spaam import SpatialDROW
    g = golden("dr_spaam_model")
    torch.manual_seed(3)
    m = SpatialDROW(num_scans=5, num_pts=56, alpha=0.5, window_size=11, pedestrian_only=True).cuda().eval()
    x = torch.from_numpy(g["x"]).cuda()

    def forwards():
        with torch.no_grad():
            pc, pr, ff = m(x)
            _, _, tmpl0, _ = m(x[:, :, 3:4], testing=True)
            c1, r1, _, f1 = m(x[:, :, 4:5], testing=True, fea_template=tmpl0)
        return pc, pr, ff, c1, r1, f1

    m.fuse_for_inference(embed="library")
    lib_out = forwards()
    m.fuse_for_inference(embed="hip")
    hip_out = forwards()
    names = ("eval_cls", "eval_reg", "eval_feat", "stream_cls", "stream_reg", "stream_feat")
    for name, got in zip(names, hip_out):
        np.testing.assert_allclose(got.cpu().numpy(), g[name], rtol=1e-3, atol=2e-3 if name.endswith("feat") else 2e-4)
    with capsys.disabled():
        print("\nembed=hip vs embed=library, max |difference|: "
              + ", ".join("%s %.3e" % (n, (a - b).abs().max().item()) for n, a, b in zip(names, hip_out, lib_out)))


# ---------------------------------------------------------------- 8. the model equals the chain written out from the ops
B, N, T, P = 1, 40, 3, 48


def _seeded_model(num_pts=P, **kw):
    """Seeded construction, BatchNorm running statistics and affine parameters randomised (a fresh model's are 0 / 1,
    which would hide a wrong fold)."""
    from planar_optical_flow_amd.src.depracted.model.dr_spaam import SpatialDROW
    torch.manual_seed(1234)
    model = SpatialDROW(num_pts=num_pts, window_size=7, **kw)
    gen = torch.Generator().manual_seed(99)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            with torch.no_grad():
                m.running_mean.copy_(torch.randn(m.num_features, generator=gen) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=gen) + 0.5)
                m.weight.copy_(torch.rand(m.num_features, generator=gen) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=gen) * 0.1)
    return model.cuda().eval()


@pytest.fixture(scope="module")
def spatial_model():
    return _seeded_model()


def _cutouts(seed, t):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn((B, N, t, P), generator=gen, device=DEV) * 2).half().float()


class _Chain:
    """The folded forward written out from the FLOAT32 trunk / gate / head ops and ``ops.attn_embed``; ``store`` is the
    storage type: an explicit rounding at every stored tensor (the identity for float32 storage)."""

    def __init__(self, ops, model, storage):
        self.ops, self.m, self.f, self.storage = ops, model, model._fused, storage

    def st(self, v):
        return v.to(self.storage)

    def block(self, name, h, pool):
        layers, start = self.f[name], 0
        if name == "conv_block_1":
            wt, sc, sh = layers[1]
            h = self.st(self.ops.conv3_first_two(h.float(), self.f["first_unit_table"], wt, sc, sh, slope1=0.1, pool=False,
                                                 negative_slope=0.1))
            start = 2
        for i in range(start, len(layers)):
            wt, sc, sh = layers[i]
            h = self.st(self.ops.conv3_bn_lrelu(h.float(), wt, sc, sh, pool=pool and i == len(layers) - 1))
        return h

    def scan_features(self, seqs):
        return self.block("conv_block_2", self.block("conv_block_1", self.st(seqs), True), True)

    def gate(self, x, t):
        gate = self.m.gate
        flat = B * N, x.shape[-2] * x.shape[-1]
        w, b = gate._folded
        emb_x, emb_t = self.ops.attn_embed(x.reshape(flat), t.reshape(flat), w, b, 0.1)     # the stored rows, un-widened
        out, band, _ = self.ops.spatial_attention(emb_x.view(B, N, 128), emb_t.view(B, N, 128), x.float().contiguous(),
                                                  t.float().contiguous(), gate._alpha, gate._window_size)
        return self.st(out), band

    def heads(self, tmpl):
        h = self.block("conv_block_3", tmpl.reshape((B * N,) + tuple(tmpl.shape[-2:])), True)
        h = self.block("conv_block_4", h, False)
        m = self.m
        cls, reg = self.ops.drow_heads(h.float(), m.conv_cls.weight, m.conv_cls.bias, m.conv_reg.weight, m.conv_reg.bias)
        return cls.view(B, N, -1), reg.view(B, N, 2)


@contextlib.contextmanager
def _no_library_linear():
    """torch.nn.functional.linear raises inside: the embed="hip" route must not reach the library GEMM."""
    def boom(*a, **k):
        raise AssertionError("the library GEMM was called on the embed='hip' route")
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch.nn.functional, "linear", boom)
        yield


@pytest.mark.parametrize("storage", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_model_equals_the_chain_of_ops(ops, spatial_model, storage):
    model = spatial_model.fuse_for_inference(storage=storage, embed="hip")
    chain = _Chain(ops, model, storage)
    with torch.no_grad():
        # the window form
        x = _cutouts(5, T)
        with _no_library_linear():
            got = model(x)
        feats = chain.scan_features(x.permute(2, 0, 1, 3).reshape(T * B * N, P))        # scan-major, as the model
        feats = feats.view(T, B, N, feats.shape[-2], feats.shape[-1])
        tmpl = feats[0]
        for t in range(1, T):
            tmpl, band = chain.gate(feats[t], tmpl)
        want = chain.heads(tmpl) + (band,)
        for g, w in zip(got, want):
            assert g.dtype == torch.float32 and g.shape == w.shape and torch.isfinite(w).all()
            assert torch.equal(g, w)
        # three streaming calls
        tmpl_m = tmpl_c = None
        for call in range(3):
            x = _cutouts(40 + call, 1)
            with _no_library_linear():
                cls, reg, tmpl_m, fused = model(x, testing=True, fea_template=tmpl_m)
            feat = chain.scan_features(x.reshape(B * N, P)).view(B, N, 256, P // 4)
            if tmpl_c is None:
                tmpl_c = feat.clone()
                _, band = chain.gate(feat, tmpl_c)
            else:
                tmpl_c, band = chain.gate(feat, tmpl_c)
            wcls, wreg = chain.heads(tmpl_c)
            assert tmpl_m.dtype == storage and cls.dtype == reg.dtype == fused.dtype == torch.float32
            for g, w in ((cls, wcls), (reg, wreg), (tmpl_m, tmpl_c), (fused, band)):
                assert torch.equal(g, w), call
        assert not torch.equal(tmpl_c, feat)             # the template really was carried and merged
    # the guard works: the library route does call the library GEMM
    model.fuse_for_inference(storage=storage, embed="library")
    with torch.no_grad(), _no_library_linear(), pytest.raises(AssertionError, match="library GEMM"):
        model(_cutouts(5, T))


# ---------------------------------------------------------------- 9. the streaming detector
@pytest.fixture(scope="module")
def stream_model():
    return _seeded_model(num_pts=56, num_scans=5, pedestrian_only=True)


_CUTOUT_KW = dict(fixed=True, centered=True, window_width=1.0, window_depth=0.5, num_cutout_pts=56, padding_val=29.99,
                  area_mode=True)


@pytest.mark.parametrize("storage", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_streaming_detector_on_the_hip_embedding(ops, stream_model, storage):
    """batch = 2, six scans with a reset in the middle: graph replay == eager detector == the model called by hand."""
    from planar_optical_flow_amd.streaming import StreamingDetector
    model = stream_model.fuse_for_inference(storage=storage, embed="hip")
    nb = 2
    scans = torch.from_numpy(synth.make_batch(seed=31, B=nb, T=6).scans).cuda()          # [2, 6, 450]
    eager, graphed = StreamingDetector(model, batch=nb, graph=False), StreamingDetector(model, batch=nb, graph=True)
    assert model._embed_route == "hip" and model._storage == storage                     # the detector did not re-fuse
    tmpl, addr = None, None
    for t in range(6):
        if t == 3:                                    # a new sequence starts
            addr = graphed.template.data_ptr()
            eager.reset(), graphed.reset()
            tmpl = None
        ce, re_ = (v.clone() for v in eager(scans[:, t]))
        cg, rg = graphed(scans[:, t])
        assert torch.equal(ce, cg) and torch.equal(re_, rg), t
        assert torch.equal(eager.template, graphed.template) and torch.equal(eager.feat_fused, graphed.feat_fused)
        with torch.no_grad():
            x = ops.cutout(scans[:, t:t + 1].contiguous(), ops.phi_table(), out_dtype=storage, **_CUTOUT_KW)
            c0, r0, tmpl, f0 = model(x, testing=True, fea_template=tmpl)
        assert torch.equal(c0, cg) and torch.equal(r0, rg) and torch.equal(f0, graphed.feat_fused), t
        assert torch.equal(tmpl, graphed.template)
        assert graphed.template.dtype == storage
        assert cg.dtype == rg.dtype == graphed.feat_fused.dtype == torch.float32
        assert cg.shape == (nb, 450, 1) and rg.shape == (nb, 450, 2)
    assert graphed._graph is not None and eager._graph is None
    assert graphed.template.data_ptr() == addr        # reset() keeps the buffer the captured graph points at
    # re-fusing with the other embedding drops the graph; the next calls still match the eager detector.  Float16
    # storage has no library route in the detector, so it goes on in float32 there.
    g_old = graphed._graph
    model.fuse_for_inference(embed="library")
    for t in (0, 1):
        ce, re_ = (v.clone() for v in eager(scans[:, t]))
        cg, rg = graphed(scans[:, t])
        assert torch.equal(ce, cg) and torch.equal(re_, rg) and torch.equal(eager.template, graphed.template), t
    assert graphed._graph is not None and graphed._graph is not g_old
    assert graphed.template.dtype == torch.float32
    g_old = graphed._graph
    model.fuse_for_inference(storage=storage, embed="hip")
    for t in (2, 3):
        ce, re_ = (v.clone() for v in eager(scans[:, t]))
        cg, rg = graphed(scans[:, t])
        assert torch.equal(ce, cg) and torch.equal(re_, rg) and torch.equal(eager.template, graphed.template), t
    assert graphed._graph is not g_old and graphed.template.dtype == storage


def test_streaming_detector_refuses_float16_with_the_library_embedding(stream_model):
    from planar_optical_flow_amd.streaming import StreamingDetector
    model = stream_model.fuse_for_inference(storage=torch.float16)
    with pytest.raises(ValueError, match="float32 storage"):
        StreamingDetector(model)
    det = StreamingDetector(stream_model.fuse_for_inference(storage=torch.float16, embed="hip"))
    model.fuse_for_inference(storage=torch.float16, embed="library")
    with pytest.raises(ValueError, match="float32 storage"):
        det(torch.full((450,), 5.0))
    model.fuse_for_inference()


@pytest.mark.parametrize("storage", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_streaming_detector_single_sensor_replays(stream_model, storage):
    """batch = 1 through five calls (eager first step, capture, three replays) against the eager detector: the scenario
    whose second replay once hung stays under test with the embedding node in the graph."""
    from planar_optical_flow_amd.streaming import StreamingDetector
    model = stream_model.fuse_for_inference(storage=storage, embed="hip")
    scans = torch.from_numpy(synth.make_batch(seed=24, B=1, T=5).scans).cuda()[0]
    graphed, eager = StreamingDetector(model, batch=1), StreamingDetector(model, batch=1, graph=False)
    for t in range(5):
        cg, rg = graphed(scans[t])
        ce, re_ = eager(scans[t])
        torch.cuda.synchronize()
        assert torch.equal(cg, ce) and torch.equal(rg, re_), t
        assert torch.equal(graphed.template, eager.template)
    assert graphed._graph is not None and graphed.template.dtype == storage
