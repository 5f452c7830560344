"""The attention backward on the GPU, held to equality.

Every case of tests/test_attention_backward_exact.py goes through both device forms -- the two-pass form
(attn_dsim_kernel<false>, attn_demb_kernel, attn_merge_kernel<W, true>) and the fused form (attn_bwd_fused_kernel<W>,
attn_dsim_finish_kernel, attn_demb_kernel) -- with g_band given and with None, and all four gradients must EQUAL the
float64 referee: the data are chosen so that nothing rounds (shown there, from the referee alone).  Then the registered
op: its autograd against the direct call for the three losses a caller can form, and strided inputs against contiguous
copies; one random-data case per window against float64 autograd at the bar of the older tests; and the forward at
embedding widths past 128."""
import numpy as np
import pytest
import torch

from test_attention_backward_exact import (CASES, GRAD_NAMES, GROUPS, band_index, case_id, case_inputs, expected,
                                           window_of)
from test_hip_parity import _torch_attention

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from planar_optical_flow_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _differences(got, want, limit=4):
    idx = (got != want).nonzero()
    head = ["%s: %r != %r" % (i, float(got[i]), float(want[i])) for i in map(tuple, idx[:limit].tolist())]
    return "%d of %d entries differ; %s" % (len(idx), want.numel(), "; ".join(head))


# ---------------------------------------------------------------- both forms on every case, bit for bit
@pytest.mark.parametrize("group", GROUPS)
def test_both_forms_equal_the_referee(ops, group):
    ran = 0
    for c in CASES:
        if c.group != group:
            continue
        ex, et, tmpl, prob, g_out, g_band = (_dev(a) for a in case_inputs(c))
        for with_band in (True, False):
            want = [_dev(a) for a in expected(c, with_band)]
            for fused in (False, True):
                got = ops.spatial_attention_backward(ex, et, tmpl, prob, g_out, g_band if with_band else None, c.alpha,
                                                     c.W, fused=fused)
                for name, a, b in zip(GRAD_NAMES, got, want):
                    assert a.dtype == torch.float32 and a.shape == b.shape
                    assert torch.equal(a, b), "%s, %s form, g_band %s, %s: %s" % (
                        case_id(c), "fused" if fused else "two-pass", "given" if with_band else "None", name,
                        _differences(a, b))
                ran += 1
    assert ran == 4 * sum(c.group == group for c in CASES)


# ---------------------------------------------------------------- the registered op
OP_SHAPES = ((2, 17, 6, 20, 7, 0.5), (3, 33, 132, 260, 15, 0.25))    # B, N, E, F, W, alpha


def _op_inputs(shape):
    B, N, E, F, W, alpha = shape
    gen = torch.Generator(device="cpu").manual_seed(40 + N)
    r = lambda *s: torch.randn(*s, generator=gen).cuda()
    return dict(ex=r(B, N, E), et=r(B, N, E), x=r(B, N, F), tmpl=r(B, N, F), g_out=r(B, N, F),
                g_band=r(B, N, window_of(W)[1]))


def _op_backward(leaves, loss, g_out, g_band, alpha, W):
    """Forward and backward through torch.ops.pof.spatial_attention -> (out, band, prob), the leaves' gradients."""
    from planar_optical_flow_amd import torch_ops  # noqa: F401  (registers torch.ops.pof.*)
    leaves = [t.detach().requires_grad_(True) for t in leaves]      # detach keeps a view's strides
    out, band, prob = torch.ops.pof.spatial_attention(*leaves, alpha, W)
    terms = []
    if loss in ("out", "both"):
        terms.append((out * g_out).sum())
    if loss in ("band", "both"):
        terms.append((band * g_band).sum())
    sum(terms).backward()
    return (out.detach(), band.detach(), prob.detach()), [t.grad for t in leaves]


@pytest.mark.parametrize("loss", ("out", "band", "both"))
@pytest.mark.parametrize("shape", OP_SHAPES, ids=lambda s: "N%d W%d" % (s[1], s[4]))
def test_registered_op_autograd_is_the_direct_call(ops, shape, loss):
    """A loss on ``out`` alone reaches the formula with g_band = None, one on ``band`` alone with g_out = None
    (set_materialize_grads(False)): either way the gradients are those of a direct call on the forward's own prob."""
    B, N, E, F, W, alpha = shape
    d = _op_inputs(shape)
    (_, _, prob), grads = _op_backward([d["ex"], d["et"], d["x"], d["tmpl"]], loss, d["g_out"], d["g_band"], alpha, W)
    go = d["g_out"] if loss != "band" else torch.zeros_like(d["tmpl"])
    gb = d["g_band"] if loss != "out" else None
    want = ops.spatial_attention_backward(d["ex"], d["et"], d["tmpl"], prob, go, gb, alpha, W)
    for name, a, b in zip(GRAD_NAMES, grads, want):
        assert a is not None and torch.equal(a, b), "%s loss, %s: %s" % (loss, name, _differences(a, b))
    if loss == "band":
        assert not grads[2].any() and not grads[3].any()           # d_x and d_tmpl are exactly zero


@pytest.mark.parametrize("shape", OP_SHAPES, ids=lambda s: "N%d W%d" % (s[1], s[4]))
def test_registered_op_takes_strided_inputs(ops, shape):
    """emb_x a transposed view, x / tmpl the first F columns of wider tensors: forward and backward are bit for bit
    those of contiguous copies (the backward op used to hand the saved views to a launcher that refuses them)."""
    B, N, E, F, W, alpha = shape
    d = _op_inputs(shape)
    pad = torch.full((B, N, 12), 7.0, device="cuda")
    ex_v = d["ex"].transpose(1, 2).contiguous().transpose(1, 2)
    x_v = torch.cat([d["x"], pad], dim=2)[..., :F]
    t_v = torch.cat([d["tmpl"], pad], dim=2)[..., :F]
    assert not ex_v.is_contiguous() and not x_v.is_contiguous() and not t_v.is_contiguous()
    assert torch.equal(ex_v, d["ex"]) and torch.equal(x_v, d["x"]) and torch.equal(t_v, d["tmpl"])
    fwd_c, grads_c = _op_backward([d["ex"], d["et"], d["x"], d["tmpl"]], "both", d["g_out"], d["g_band"], alpha, W)
    fwd_v, grads_v = _op_backward([ex_v, d["et"], x_v, t_v], "both", d["g_out"], d["g_band"], alpha, W)
    for name, a, b in zip(("out", "band", "prob"), fwd_v, fwd_c):
        assert torch.equal(a, b), "forward %s: %s" % (name, _differences(a, b))
    for name, a, b in zip(GRAD_NAMES, grads_v, grads_c):
        assert a is not None and torch.equal(a, b), "%s: %s" % (name, _differences(a, b))


# ---------------------------------------------------------------- random data at the seams, device-forward prob
@pytest.mark.parametrize("W", (1, 3, 5, 7, 9, 11, 13, 15))
def test_random_data_at_the_seams_vs_float64_autograd(ops, W):
    """N = 17 (a last unit of one point), E = 132 (a chunk of four columns), F = 260 (a wave's columns and one float4),
    weights from the device's own forward: every gradient of both forms within 2e-4 of the referee's largest entry,
    the bar of test_attention_backward_under_saturation.  The exact cases hold the index logic; this shows that the
    forward's weights and the backward still meet at shapes the older tests never ran."""
    B, N, E, F, alpha = 2, 17, 132, 260, 0.5
    gen = torch.Generator(device="cpu").manual_seed(900 + W)
    r = lambda *s: torch.randn(*s, generator=gen)
    ex, et = 0.3 * r(B, N, E), 0.3 * r(B, N, E)
    x, tmpl, g_out, g_band = r(B, N, F), r(B, N, F), r(B, N, F), r(B, N, W)
    leaves = [t.double().requires_grad_(True) for t in (ex, et, x, tmpl)]
    out, band = _torch_attention(*leaves, alpha, W)
    ((out * g_out.double()).sum() + (band * g_band.double()).sum()).backward()
    want = [t.grad for t in leaves]
    dev = [t.cuda() for t in (ex, et, x, tmpl, g_out, g_band)]
    _, _, prob = ops.spatial_attention(dev[0], dev[1], dev[2], dev[3], alpha, W)
    for fused in (False, True):
        got = ops.spatial_attention_backward(dev[0], dev[1], dev[3], prob, dev[4], dev[5], alpha, W, fused=fused)
        ratios = []
        for name, a, b in zip(GRAD_NAMES, got, want):
            err, scale = float((a.double().cpu() - b).abs().max()), float(b.abs().max())
            ratios.append((name, err / scale))
        print("W=%d %s: " % (W, "fused" if fused else "two-pass") + ", ".join("%s %.2e" % r for r in ratios))
        for name, ratio in ratios:
            assert ratio <= 2e-4, (W, fused, name, ratio)


# ---------------------------------------------------------------- forward, embeddings wider than 128
@pytest.mark.parametrize("E", (129, 132, 260))
def test_forward_past_128_embedding_columns(ops, E):
    """Embeddings in multiples of 1/8 within [-0.5, 0.5]: the band is bit for bit the float64 dot products (E = 129
    through the LDS-tiled form for E % 4 != 0, which takes it: its 44 KB of LDS are inside its 60 KB bound), prob is 0
    on clamped slots and within 1e-6 of the float64 softmax (the bar of test_attention_forward_under_saturation)."""
    B, N, F, W, alpha = 2, 19, 8, 11, 0.5
    rng = np.random.default_rng(300 + E)
    ex, et = (rng.integers(-4, 5, (B, N, E)) / 8.0 for _ in range(2))
    x, tmpl = rng.standard_normal((B, N, F)), rng.standard_normal((B, N, F))
    cols, valid = band_index(N, W)
    band64 = np.einsum("bie,bike->bik", ex, et[:, cols])
    e = np.where(valid[None], np.exp(band64 - np.where(valid[None], band64, -np.inf).max(-1, keepdims=True)), 0.0)
    prob64 = e / e.sum(-1, keepdims=True)
    _, band, prob = ops.spatial_attention(_dev(ex), _dev(et), _dev(x), _dev(tmpl), alpha, W)
    band, prob = band.cpu().numpy(), prob.cpu().numpy()
    assert np.array_equal(band.astype(np.float64), band64), np.argwhere(band != band64)[:4]
    assert not prob[:, ~valid].any()
    np.testing.assert_allclose(prob, prob64, rtol=0, atol=1e-6)
